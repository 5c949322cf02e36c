// rs_tables_dump -- the host side of the Reed-Solomon code (viterbidecodercpp_amd/csrc/rs_tables.hpp) as a program of its own, for
// tests/test_rs_cpu.py: no HIP, no library, nothing but the header.
//   rs_tables_dump            reads lines "gfpoly fcr prim nroots pad dual_basis" from standard input and answers each with one line:
//                             "invalid <what rs_params_invalid says>" or "ok <the RS_TABLE_BYTES bytes of the blob as hex>"
//   rs_tables_dump geometry   prints "nroots n R2 G seg base" for every nroots 2 .. 64 and every n from nroots + 1 to 255
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../viterbidecodercpp_amd/csrc/rs_tables.hpp"

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "geometry") == 0) {
        for (uint32_t nroots = 2; nroots <= 64; ++nroots)
            for (uint32_t n = nroots + 1; n <= 255; ++n) {
                const vit::RsGeometry g = vit::rs_geometry(nroots, n);
                std::printf("%u %u %u %u %u %u\n", nroots, n, g.R2, g.G, g.seg, g.base);
            }
        return 0;
    }
    if (argc > 1) {
        std::fprintf(stderr, "usage: %s [geometry]\n", argv[0]);
        return 2;
    }
    vit_hip_rs_params p;
    while (std::scanf("%u %u %u %u %u %u", &p.gfpoly, &p.fcr, &p.prim, &p.nroots, &p.pad, &p.dual_basis) == 6) {
        if (const char* why = vit::rs_params_invalid(&p)) {
            std::printf("invalid %s\n", why);
            continue;
        }
        std::vector<uint8_t> blob(vit::RS_TABLE_BYTES);           // on the heap: a write past the end is seen by the sanitizer
        vit::rs_build_tables(&p, blob.data());
        std::printf("ok ");
        for (uint8_t b : blob) std::printf("%02x", b);
        std::printf("\n");
    }
    return 0;
}
