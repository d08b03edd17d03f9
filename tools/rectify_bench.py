"""Device time of the rectification front end, HIP events around the device
entry points on one stream: 5 warm-up iterations + 50 timed, the median reported.  One
iteration is --reps back-to-back launches between two events (a single 10-microsecond
launch would measure the events), the figure is per launch.
    python tools/rectify_bench.py [--out profiles/rectify/rectify_bench.jsonl] [--no-chain] [--no-cpu]
Per shape (1280x720 and 1242x375, 3 channels):
  map        k_rectify_map, one camera
  remap      k_remap_u8, gray only and gray + BGR, 2 and 16 images sharing one map pair, with
             the achieved bytes/s over the compulsory bytes: 8 B/px of maps (once per launch)
             + per image 3 B/px of source + 1 or 4 B/px of output
  chain      StereoRectifier.compute_disparity (raw BGR frames in) against compute_disparity
             on pre-rectified host grays, wall time per pair, settings.ini values (D = 160)
  cpu        the numpy restatement tests/rectify_np.py on this host's CPU (there is no cv2 to time)
One JSON object per line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(720, 1280), (375, 1242)]
WARMUP, TIMED = 5, 50


def _rig(W, H):
    rng = np.random.default_rng(5)
    f = 0.9 * W
    K = [np.array([[f + rng.uniform(-5, 5), 0, W / 2 + rng.uniform(-3, 3)],
                   [0, f + rng.uniform(-5, 5), H / 2 + rng.uniform(-3, 3)], [0, 0, 1.0]]) for _ in range(2)]
    dist = np.array([-0.05, 0.01, 0.001, -0.0005, 0.002])
    return K[0], K[1], dist, rng.uniform(-0.02, 0.02, 3), np.array([-0.12, 0.002, -0.001])


def _device_us(fn, reps):
    import torch

    ts = []
    for it in range(WARMUP + TIMED):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        if it >= WARMUP:
            ts.append(a.elapsed_time(b) * 1e3 / reps)
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-chain", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    import torch

    import stereo_match_amd as sm
    from stereo_match_amd import _lib, rectify, synthetic

    dev = torch.device("cuda", 0)
    eng = _lib.engine(0)
    st = torch.cuda.Stream(device=dev)
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    for H, W in SHAPES:
        K1, K2, dist, om, T = _rig(W, H)
        R1, R2, P1, P2, Q, _, _ = rectify.stereoRectify(K1, dist, K2, dist, (W, H), om, T)
        cam = rectify._rectify_cam(K1, dist, R1, P1)
        npx = H * W
        rng = np.random.default_rng(1)
        with torch.cuda.stream(st):
            eng.set_stream(st.cuda_stream)
            mx = torch.empty((H, W), dtype=torch.float32, device=dev)
            my = torch.empty_like(mx)
            us, lo = _device_us(lambda: eng.rectify_map_device(cam, H, W, mx.data_ptr(), my.data_ptr()), args.reps)
            emit(what="map", H=H, W=W, us=round(us, 2), us_min=round(lo, 2), GBps=round(8 * npx / us / 1e3, 1))
            for nimg in (2, 16):
                src = torch.from_numpy(rng.integers(0, 256, (nimg, H, W, 3), dtype=np.uint8)).to(dev)
                dst = torch.empty((nimg, H, W, 3), dtype=torch.uint8, device=dev)
                gray = torch.empty((nimg, H, W), dtype=torch.uint8, device=dev)
                for outputs, d_dst, out_b in (("gray", None, 1), ("gray+bgr", dst.data_ptr(), 4)):
                    us, lo = _device_us(lambda: eng.remap_batch_device(
                        src.data_ptr(), nimg, npx * 3, H, W, 3 * W, 3, mx.data_ptr(), my.data_ptr(), H, W, d_dst,
                        gray.data_ptr()), args.reps)
                    nbytes = npx * (8 + nimg * (3 + out_b))
                    emit(what="remap", H=H, W=W, nimg=nimg, outputs=outputs, us=round(us, 2), us_min=round(lo, 2),
                         us_per_image=round(us / nimg, 2), compulsory_bytes=nbytes,
                         GBps=round(nbytes / us / 1e3, 1))
                us, lo = _device_us(lambda: eng.bgr2gray_batch_device(src.data_ptr(), nimg, npx * 3, H, W, 3 * W,
                                                                      gray.data_ptr()), args.reps)
                emit(what="bgr2gray", H=H, W=W, nimg=nimg, us=round(us, 2), us_min=round(lo, 2),
                     GBps=round(npx * nimg * 4 / us / 1e3, 1))
            st.synchronize()
        eng.set_stream(None)

        if not args.no_chain:
            s = dict(sm.DEFAULT_SETTINGS, window_size=5, num_disparities=160)
            gl, gr, _ = synthetic.random_dot_pair(H, W, 160, seed=77)
            vis_l, vis_r = np.ascontiguousarray(np.stack([gl] * 3, -1)), np.ascontiguousarray(np.stack([gr] * 3, -1))
            sr = rectify.StereoRectifier(K1, dist, K2, dist, (W, H), om, T)

            def wall(fn):
                ts = []
                for it in range(WARMUP + 20):
                    t0 = time.perf_counter()
                    fn()
                    if it >= WARMUP:
                        ts.append(time.perf_counter() - t0)
                return round(float(np.median(ts)) * 1e3, 3)

            ms_chain = wall(lambda: sr.compute_disparity(vis_l, vis_r, s))
            eng.set_stream(None)
            ms_gray = wall(lambda: sm.compute_disparity(gl, gr, s))
            emit(what="chain", H=H, W=W, D=160, ms_per_pair_raw_frames=ms_chain, ms_per_pair_host_grays=ms_gray,
                 front_end_adds_ms=round(ms_chain - ms_gray, 3))

        if not args.no_cpu:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import rectify_np

            img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            t0 = time.perf_counter()
            ex, ey = rectify_np.rectify_map(K1, dist, np.array(cam.iR[:]), H, W)
            t1 = time.perf_counter()
            r = rectify_np.remap(img, ex, ey)
            t2 = time.perf_counter()
            rectify_np.bgr2gray(r)
            t3 = time.perf_counter()
            emit(what="cpu_numpy_restatement", H=H, W=W, map_ms=round((t1 - t0) * 1e3, 1),
                 remap_ms=round((t2 - t1) * 1e3, 1), gray_ms=round((t3 - t2) * 1e3, 1))

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
