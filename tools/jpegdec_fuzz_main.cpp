// jpegdec_fuzz_main.cpp — the JPEG decoder's CPU twin (sm_jpegdec.hpp) under the
// host compiler's sanitizers: a stand-alone program that launches nothing, nothing preloaded.
//
//   jpegdec_fuzz SEED file.jpg [file.jpg ...]
//
// For each file: the file itself (must decode), its truncations (every length of a file of up to
// 4096 bytes, every 13th of a larger one; each must be rejected) and 2000 single-byte mutations
// anywhere in the file (any verdict; the sanitizers watch every read and write).  The file and the
// output buffer are exact-size heap blocks, so one byte out of bounds is a report.  Exit 0 when
// all of it ran.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <vector>

#include "sm_jpegdec.hpp"

namespace {

using namespace smk;

// decode `n` bytes held in an exact-size block to BGR; returns the status
int decode(const uint8_t* src, size_t n)
{
    std::unique_ptr<uint8_t[]> file(new uint8_t[n ? n : 1]);
    std::memcpy(file.get(), src, n);
    JdDesc d;
    const int st = jd_parse(file.get(), n, d);
    if (st) return st;
    JdArgs a{};
    a.nimg = 1, a.H = (int)d.H, a.W = (int)d.W, a.ncomp = d.ncomp, a.hs = d.hs, a.vs = d.vs;
    a.out_ch = 3, a.y_only = d.ncomp == 1, a.keep = 0;
    jd_geometry(a);
    const size_t row = (size_t)d.W * 3;
    std::unique_ptr<uint8_t[]> out(new uint8_t[row * d.H]);
    a.out = out.get(), a.row_stride = row;
    const uint64_t off = 0, size = n;
    a.files = file.get(), a.offsets = &off, a.sizes = &size, a.desc = &d, a.max_file = (uint32_t)n;
    uint32_t nsub = 0;
    return jpegdec_host(a, nsub);
}

int fuzz(const std::vector<uint8_t>& file, std::mt19937& rng, const char* name)
{
    const int st = decode(file.data(), file.size());
    if (st) {
        std::fprintf(stderr, "%s: the unmodified file is rejected: %s\n", name, jpegdec_message(st));
        return 1;
    }
    const size_t step = file.size() <= 4096 ? 1 : 13;
    for (size_t n = 0; n < file.size(); n += step)
        if (decode(file.data(), n) == JD_OK) {
            std::fprintf(stderr, "%s: accepted when cut to %zu bytes\n", name, n);
            return 1;
        }
    int rejected = 0;
    for (int k = 0; k < 2000; ++k) {
        std::vector<uint8_t> m = file;
        m[rng() % m.size()] ^= (uint8_t)(1u + rng() % 255u);
        rejected += decode(m.data(), m.size()) != JD_OK;
    }
    std::printf("%s: %zu bytes, %zu truncations rejected, %d of 2000 mutations rejected\n", name, file.size(),
                (file.size() + step - 1) / step, rejected);
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 3) {
        std::fprintf(stderr, "usage: jpegdec_fuzz SEED file.jpg [file.jpg ...]\n");
        return 2;
    }
    std::mt19937 rng((uint32_t)std::strtoul(argv[1], nullptr, 10));
    int rc = 0;
    for (int i = 2; i < argc; ++i) {
        std::FILE* f = std::fopen(argv[i], "rb");
        if (!f) {
            std::fprintf(stderr, "cannot open %s\n", argv[i]);
            return 2;
        }
        std::vector<uint8_t> file;
        uint8_t buf[4096];
        size_t n;
        while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) file.insert(file.end(), buf, buf + n);
        std::fclose(f);
        rc |= fuzz(file, rng, argv[i]);
    }
    return rc;
}
