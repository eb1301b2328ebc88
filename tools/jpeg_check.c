// The JPEG core (mav-detection_amd/csrc/jpeg_core.h) on the host under AddressSanitizer and UBSan: a stand-alone program, never loaded
// into python and never run on a GPU.  Built by `make -C mav-detection_amd/csrc jpeg_check` with the host C++ compiler (the core is a
// header of templates, so this file is compiled as C++).
//
//     jpeg_check FILE      FILE: python tests/jpeg_cases.py --dump FILE
//
// Every case goes through the parser and the host decoder in all three output formats: a valid case must give the table's BGR pixels,
// a refused case its code and an all-zero output.  Then every valid file is cut at every length and has every byte behind SOI flipped
// in turn (a large file: at some 1500 places); whatever the verdict, the sanitizers must stay silent and a failed image must be all zero.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "jpeg_core.h"

static long decodes = 0;

static uint32_t rd32(FILE* f)
{
    uint8_t b[4];
    if (fread(b, 1, 4, f) != 4) { fprintf(stderr, "short read\n"); exit(2); }
    return b[0] | (b[1] << 8) | (b[2] << 16) | ((uint32_t)b[3] << 24);
}
static std::vector<uint8_t> rdn(FILE* f, size_t n)
{
    std::vector<uint8_t> v(n);
    if (n && fread(v.data(), 1, n, f) != n) { fprintf(stderr, "short read\n"); exit(2); }
    return v;
}
// parse + decode of arbitrary bytes; returns the decoder's code, or -(parser's code); out: the BGR picture when there is one
static int run(const uint8_t* file, size_t n, int format, std::vector<uint8_t>* out, mav_jpeg_info* info)
{
    char why[160];
    // an exact-size copy, so that a read behind the file's end is a read behind an allocation
    std::vector<uint8_t> copy(file, file + n);
    const int rc = jc_parse(copy.data(), n, info, why, sizeof why);
    if (rc) return -rc;
    if ((uint64_t)info->W * info->H > (1u << 22)) return -100;          // a flipped size byte: too large a picture to be worth decoding
    out->assign((size_t)info->W * info->H * jc_out_channels(info->components, format), 0xAB);
    mav_jpeg_status st;
    if (jc_decode_host(copy.data(), n, info, format, out->data(), &st) != 0) { fprintf(stderr, "out of memory\n"); exit(2); }
    decodes++;
    if (st.code)
        for (size_t i = 0; i < out->size(); i++)
            if ((*out)[i]) { fprintf(stderr, "a failed image (code %d) is not all zero\n", st.code); exit(1); }
    return st.code;
}

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: jpeg_check FILE\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const std::vector<uint8_t> magic = rdn(f, 4);
    if (memcmp(magic.data(), "JPGC", 4)) { fprintf(stderr, "not a case table\n"); return 2; }
    const uint32_t count = rd32(f);
    int failed = 0, valid = 0, refused = 0;
    for (uint32_t k = 0; k < count; k++) {
        const std::vector<uint8_t> name_b = rdn(f, rd32(f));
        const std::string name(name_b.begin(), name_b.end());
        const int code = (int)rd32(f);
        const int by_parser = rdn(f, 1)[0];
        const std::vector<uint8_t> file = rdn(f, rd32(f));
        const uint32_t H = rd32(f), W = rd32(f);
        const std::vector<uint8_t> want = rdn(f, rd32(f));
        mav_jpeg_info info;
        std::vector<uint8_t> out;
        for (int format = 0; format < 3; format++) {
            const int got = run(file.data(), file.size(), format, &out, &info);
            const int expect = by_parser ? -code : code;
            if (got != expect) { fprintf(stderr, "%s: format %d: code %d, expected %d\n", name.c_str(), format, got, expect); failed++; }
            if (!code && format == MAV_JPEG_OUT_BGR && (info.W != (int)W || info.H != (int)H || out != want)) {
                fprintf(stderr, "%s: the BGR pixels differ from the table's\n", name.c_str());
                failed++;
            }
        }
        code ? refused++ : valid++;
        if (code) continue;
        const size_t step = file.size() / 1500 + 1;                       // every byte of a small file, some 1500 of a large one
        for (size_t cut = 0; cut < file.size(); cut += step) run(file.data(), cut, MAV_JPEG_OUT_BGR, &out, &info);
        std::vector<uint8_t> m(file);
        for (size_t i = 2; i < m.size(); i += step) {
            m[i] ^= 0xFF;
            run(m.data(), m.size(), (int)(i % 3), &out, &info);
            m[i] = (uint8_t)(file[i] ^ (1u << (i % 8)));
            run(m.data(), m.size(), (int)(i % 3), &out, &info);
            m[i] = file[i];
        }
    }
    fclose(f);
    printf("jpeg_check: %d valid and %d refused cases, %ld decodes of cut and flipped files, %d failures\n", valid, refused, decodes, failed);
    return failed ? 1 : 0;
}
