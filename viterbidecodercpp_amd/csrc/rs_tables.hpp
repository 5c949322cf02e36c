// rs_tables.hpp -- the host side of a Reed-Solomon code over GF(256) (vit_hip_rs_create): the parameter rule and the tables the kernel
// of kernels_rs.hpp reads.  Plain C++ with no HIP in it, so the same source also builds into a host program of its own.
//   blob layout, RS_TABLE_BYTES bytes: exp[512] (exp[i] = alpha^(i mod 255), so a sum of two logarithms needs no reduction),
//   log[256] (log[0] is never read), to_conv[256] (stored byte -> conventional), to_dual[256] (conventional -> stored byte); the last
//   two are the identity without the dual basis.
#pragma once
#include <stdint.h>

#include "../../include/vit_hip.h"

namespace vit {

constexpr uint32_t RS_EXP = 0, RS_LOG = 512, RS_TO_CONV = 768, RS_TO_DUAL = 1024, RS_TABLE_BYTES = 1280;

inline uint32_t rs_gcd(uint32_t a, uint32_t b) { while (b) { const uint32_t t = a % b; a = b; b = t; } return a; }

// fills exp / log; false when x is not a primitive element of GF(2)[x] / gfpoly
inline bool rs_field(uint32_t gfpoly, uint8_t* exp_t, uint8_t* log_t) {
    if (gfpoly < 0x100 || gfpoly > 0x1FF) return false;
    bool seen[256] = {false};
    uint32_t v = 1;
    for (uint32_t i = 0; i < 255; ++i) {
        if (seen[v]) return false;                 // the powers of x repeat before all 255 non-zero elements appeared
        seen[v] = true;
        exp_t[i] = (uint8_t)v;
        log_t[v] = (uint8_t)i;
        v <<= 1;
        if (v & 0x100) v ^= gfpoly;
    }
    if (v != 1) return false;
    for (uint32_t i = 255; i < 512; ++i) exp_t[i] = exp_t[i - 255];
    log_t[0] = 0;
    return true;
}

// what is wrong with the parameters, or nullptr
inline const char* rs_params_invalid(const vit_hip_rs_params* p) {
    if (!p) return "NULL parameters";
    if (p->gfpoly < 0x100 || p->gfpoly > 0x1FF) return "gfpoly must have its x^8 term and no higher one";
    if (p->nroots < 2 || p->nroots > 64) return "nroots must be 2 .. 64";
    if (p->pad >= 255 || 255 - p->pad <= p->nroots) return "n = 255 - pad must exceed nroots";
    if (p->prim == 0 || p->prim > 254 || rs_gcd(p->prim, 255) != 1) return "prim must be 1 .. 254 and coprime to 255";
    if (p->fcr > 254) return "fcr must be 0 .. 254";
    if (p->dual_basis > 1) return "dual_basis must be 0 or 1";
    if (p->dual_basis && p->gfpoly != 0x187) return "the dual basis is defined for gfpoly 0x187 only";
    uint8_t e[512], l[256];
    if (!rs_field(p->gfpoly, e, l)) return "gfpoly is not primitive";
    return nullptr;
}

// how the kernel cuts a codeword's 256-byte slot for the syndromes (kernels_rs.hpp): R2 lanes per segment, the power of two at or above
// nroots; G = 64 / R2 segments of seg bytes, a multiple of 4; base = G * seg - n zero bytes in front.  nroots 2 .. 64, nroots < n <= 255
struct RsGeometry {
    uint32_t R2, G, seg, base;
};

inline RsGeometry rs_geometry(uint32_t nroots, uint32_t n) {
    RsGeometry g{};
    g.R2 = 2;
    while (g.R2 < nroots) g.R2 *= 2;
    g.G = 64 / g.R2;
    g.seg = ((n + g.G - 1) / g.G + 3) / 4 * 4;                     // G * seg <= 256: 256 / G is a multiple of 4
    g.base = g.G * g.seg - n;
    return g;
}

// the blob of a code rs_params_invalid accepted
inline void rs_build_tables(const vit_hip_rs_params* p, uint8_t* blob) {
    uint8_t* exp_t = blob + RS_EXP;
    uint8_t* log_t = blob + RS_LOG;
    rs_field(p->gfpoly, exp_t, log_t);
    for (uint32_t x = 0; x < 256; ++x) blob[RS_TO_CONV + x] = blob[RS_TO_DUAL + x] = (uint8_t)x;
    if (!p->dual_basis) return;
    // CCSDS 131.0-B: bit 7-i of the stored byte is Tr(x * beta^i), beta = alpha^117; Tr(y) = y + y^2 + ... + y^128 is 0 or 1
    for (uint32_t x = 0; x < 256; ++x) {
        uint32_t stored = 0;
        for (uint32_t i = 0; i < 8; ++i) {
            uint32_t tr = 0;
            if (x) {
                const uint32_t ly = (log_t[x] + 117u * i) % 255u;
                for (uint32_t k = 0, m = 1; k < 8; ++k, m = m * 2 % 255) tr ^= exp_t[ly * m % 255u];
            }
            stored |= (tr & 1u) << (7 - i);
        }
        blob[RS_TO_DUAL + x] = (uint8_t)stored;
        blob[RS_TO_CONV + stored] = (uint8_t)x;
    }
}

}  // namespace vit
