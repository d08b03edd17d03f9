// pngdec_fuzz_main.cpp — the PNG decoder's CPU twin (sm_pngdec.hpp) under the host
// compiler's sanitizers: a stand-alone program that launches nothing, nothing preloaded.
//
//   pngdec_fuzz SEED [file.png ...]
//
// Makes small files with the package's own encoder twin (gray, BGR and 16-bit), takes the files
// named on the command line as well, and decodes, for each: the file itself (must decode), its
// truncations (every length of a file of up to 4096 bytes, every 13th of a larger one; each must
// be rejected), and 2000 single-byte mutations of its IDAT data with the chunk CRCs recomputed (any
// verdict; the sanitizers watch every read and write).  The files and the output buffer are
// exact-size heap blocks, so one byte out of bounds is a report.  Exit 0 when all of it ran.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <vector>

#include "sm_pngdec.hpp"

namespace {

using namespace smk;

// decode `n` bytes held in an exact-size block; returns the status
int decode(const uint8_t* src, size_t n, uint32_t* path = nullptr)
{
    std::unique_ptr<uint8_t[]> file(new uint8_t[n ? n : 1]);
    std::memcpy(file.get(), src, n);
    PdHdr h{};
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    if (n < 8 || std::memcmp(file.get(), sig, 8) != 0) return PD_E_SIG;
    if (n < 33) return PD_E_TRUNC;
    if (pd_be32(file.get() + 8) != 13u || std::memcmp(file.get() + 12, "IHDR", 4) != 0) return PD_E_IHDR;
    const int st = pd_ihdr(file.get() + 16, h);
    if (st) return st;
    PdArgs a{};
    a.nimg = 1, a.H = (int)h.H, a.W = (int)h.W, a.file_ch = h.channels, a.depth = h.depth, a.bpp = h.channels * h.depth / 8;
    a.rowbytes = h.W * (uint32_t)a.bpp, a.stream_len = ((uint64_t)a.rowbytes + 1) * h.H, a.stream_stride = a.stream_len;
    a.nseg = (uint32_t)((a.stream_len + PNG_SEG - 1) / PNG_SEG);
    a.maxpar = 2u * (uint32_t)((a.stream_len + PNGDEC_CAP - 1) / PNGDEC_CAP) + 4u;
    a.kind = h.depth == 16 ? PD_OUT_U16 : PD_OUT_U8;
    a.out_ch = h.channels == 1 ? 1 : 3;
    const size_t row = (size_t)h.W * (h.depth == 16 ? 2 : (size_t)a.out_ch);
    std::unique_ptr<uint8_t[]> out(new uint8_t[row * h.H]);
    a.out = out.get(), a.row_stride = row;
    const uint64_t off = 0, size = n;
    a.files = file.get(), a.offsets = &off, a.sizes = &size;
    uint32_t p = 0;
    const int rc = pngdec_host(a, p);
    if (path) *path = p;
    return rc;
}

void fix_crcs(std::vector<uint8_t>& f)
{
    size_t pos = 8;
    while (pos + 12 <= f.size()) {
        const uint32_t len = pd_be32(&f[pos]);
        if (len > f.size() - pos - 12) break;
        uint32_t reg = 0xFFFFFFFFu;
        for (size_t i = pos + 4; i < pos + 8 + len; ++i) reg = png_crc_byte(reg, f[i]);
        png_put_be32(&f[pos + 8 + len], ~reg);
        pos += 12 + len;
    }
}

// offsets of the bytes of all IDAT data
std::vector<size_t> idat_bytes(const std::vector<uint8_t>& f)
{
    std::vector<size_t> v;
    size_t pos = 8;
    while (pos + 12 <= f.size()) {
        const uint32_t len = pd_be32(&f[pos]);
        if (len > f.size() - pos - 12) break;
        if (std::memcmp(&f[pos + 4], "IDAT", 4) == 0)
            for (uint32_t i = 0; i < len; ++i) v.push_back(pos + 8 + i);
        pos += 12 + len;
    }
    return v;
}

int fuzz(const std::vector<uint8_t>& file, std::mt19937& rng, const char* name)
{
    uint32_t path = 0;
    int st = decode(file.data(), file.size(), &path);
    if (st) {
        std::fprintf(stderr, "%s: the unmodified file is rejected: %s\n", name, pngdec_message(st));
        return 1;
    }
    const size_t step = file.size() <= 4096 ? 1 : 13;  // every length of a small file
    for (size_t n = 0; n < file.size(); n += step)
        if (decode(file.data(), n) == PD_OK) {
            std::fprintf(stderr, "%s: accepted when cut to %zu bytes\n", name, n);
            return 1;
        }
    const std::vector<size_t> at = idat_bytes(file);
    int rejected = 0;
    for (int k = 0; k < 2000 && !at.empty(); ++k) {
        std::vector<uint8_t> m = file;
        m[at[rng() % at.size()]] ^= (uint8_t)(1u + rng() % 255u);
        fix_crcs(m);
        rejected += decode(m.data(), m.size()) != PD_OK;
    }
    std::printf("%s: %zu bytes, path %u, %zu truncations rejected, %d of 2000 mutations rejected\n", name, file.size(), path,
                (file.size() + step - 1) / step, rejected);
    return 0;
}

std::vector<uint8_t> own_file(std::mt19937& rng, int kind, int channels, int H, int W)
{
    const int esz = kind == PNG_SRC_U16 ? 2 : 1;
    std::vector<uint8_t> img((size_t)H * W * channels * esz);
    uint8_t v = 0;
    for (auto& b : img) {
        if (rng() % 3 == 0) v = (uint8_t)(rng() % 40);
        b = v;
    }
    PngArgs s{};
    s.img = img.data(), s.row_stride = (size_t)W * channels * esz, s.H = H, s.W = W;
    s.kind = kind, s.channels = channels, s.filter = -1;
    s.depth = 8 * esz, s.out_channels = channels, s.bpp = channels * esz;
    s.rowbytes = (uint32_t)(W * s.bpp), s.stream_len = ((uint64_t)s.rowbytes + 1) * H;
    s.nseg = (uint32_t)((s.stream_len + PNG_SEG - 1) / PNG_SEG);
    std::vector<uint8_t> file;
    png_encode_host(s, file);
    return file;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 2) {
        std::fprintf(stderr, "usage: pngdec_fuzz SEED [file.png ...]\n");
        return 2;
    }
    std::mt19937 rng((uint32_t)std::strtoul(argv[1], nullptr, 10));
    int rc = 0;
    rc |= fuzz(own_file(rng, PNG_SRC_U8, 1, 19, 23), rng, "own gray");
    rc |= fuzz(own_file(rng, PNG_SRC_U8, 3, 7, 11), rng, "own bgr");
    rc |= fuzz(own_file(rng, PNG_SRC_U16, 1, 5, 9), rng, "own gray16");
    rc |= fuzz(own_file(rng, PNG_SRC_U8, 1, 3, 13000), rng, "own two segments");
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
