"""Size quality of the PNG coder, measured with the CPU twin (no GPU needed):
the IDAT bytes of sm_png_encode_host against zlib on the SAME filtered stream, at level 6 (what
cv2.imwrite and Pillow use by default) and at level 1 with Z_RLE (runs at distance 1 only, the
closest relative of this coder), each as one stream and as 32 KiB pieces joined by sync flushes
(this coder's framing).
    python tools/png_size.py [--out profiles/png/size.jsonl]
Inputs: a synthetic 1280x720 frame (stereo_match_amd/synthetic.py under a ramp) as BGR and gray,
the disparity maps of the GPU goldens (tests/golden/*.npz, `expected`) and a jittered KITTI-size
map, each as the KITTI 16-bit file and as the min-max uint8 picture.  One JSON object per line."""
import argparse
import glob
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SEG = 32768


def zl(stream, level, strategy, pieces):
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    if not pieces:
        return len(c.compress(stream) + c.flush())
    n = 0
    for k in range(0, len(stream), SEG):
        n += len(c.compress(stream[k:k + SEG]) + c.flush(zlib.Z_FULL_FLUSH))
    return n + len(c.flush())


def line(name, kind, png):
    from png_bench import stream_of

    stream = stream_of(png)
    nseg = -(-len(stream) // SEG)
    idat = len(png) - 57 - 12 * nseg
    return dict(what="png_size", input=name, kind=kind, stream_bytes=len(stream), segments=nseg, idat_bytes=idat,
                file_bytes=len(png), zlib6=zl(stream, 6, zlib.Z_DEFAULT_STRATEGY, False),
                zlib6_pieces=zl(stream, 6, zlib.Z_DEFAULT_STRATEGY, True), zlib_rle=zl(stream, 1, zlib.Z_RLE, False),
                zlib_rle_pieces=zl(stream, 1, zlib.Z_RLE, True),
                over_zlib_rle_pieces=round(idat / zl(stream, 1, zlib.Z_RLE, True), 3),
                over_zlib6=round(idat / zl(stream, 6, zlib.Z_DEFAULT_STRATEGY, False), 3))


def main():
    import stereo_match_amd as sma
    from png_bench import frame, kitti_map

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []
    f = frame()
    lines.append(line("synthetic_frame_720p", "bgr", sma.imencode_png_host(f)))
    lines.append(line("synthetic_frame_720p", "gray", sma.imencode_png_host(np.ascontiguousarray(f[..., 1]))))
    maps = [("jittered_kitti_size_map", kitti_map())]
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz"))):
        base = os.path.basename(path)[:-4]
        if base.startswith(("vol_", "wls_")):
            continue
        z = np.load(path, allow_pickle=False)
        if "expected" in z.files and z["expected"].dtype == np.int16:
            maps.append(("golden_" + base, z["expected"]))
    for name, d in maps:
        lines.append(line(name, "kitti_u16", sma.encode_disparity_png(d, "kitti", host=True)))
        lines.append(line(name, "minmax_u8", sma.encode_disparity_png(d, "u8", host=True)))
    text = "\n".join(json.dumps(x) for x in lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            fo.write(text)


if __name__ == "__main__":
    main()
