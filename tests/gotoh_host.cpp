// gotoh_host.cpp - the exact gap-affine global alignment score by plain dynamic programming (Gotoh 1982): three matrices, one
// row each, int32.  The independent yardstick of the WFA tests: it shares nothing with the oracle's or the product's wavefront
// code - no wavefronts, no diagonals, no heuristics.  Test infrastructure; built by tests/gotoh.py.
//
//   M[i][j]  best cost of q[0..i) against t[0..j) ending in a column that pairs q[i-1] with t[j-1]
//   I[i][j]  ... ending in a gap that consumes t[j-1] only
//   D[i][j]  ... ending in a gap that consumes q[i-1] only
//   mismatch x, a gap of n bases o + n * e; bytes are compared as bytes.
#include <stdint.h>

#include <algorithm>
#include <vector>

extern "C" int32_t gotoh_score(const uint8_t *q, int32_t qlen, const uint8_t *t, int32_t tlen, int32_t x, int32_t o, int32_t e) {
    const int32_t INF = INT32_MAX / 4;
    std::vector<int32_t> M((size_t)tlen + 1), I((size_t)tlen + 1), D((size_t)tlen + 1);
    M[0] = 0;
    I[0] = D[0] = INF;
    for (int32_t j = 1; j <= tlen; j++) {
        M[j] = D[j] = INF;
        I[j] = o + e * j;
    }
    for (int32_t i = 1; i <= qlen; i++) {
        int32_t diag_m = M[0], diag_i = I[0], diag_d = D[0]; // row i-1, column j-1
        M[0] = I[0] = INF;
        D[0] = o + e * i;
        for (int32_t j = 1; j <= tlen; j++) {
            const int32_t up_m = M[j], up_i = I[j], up_d = D[j]; // row i-1, column j
            const int32_t sub = q[i - 1] == t[j - 1] ? 0 : x;
            M[j] = std::min(diag_m, std::min(diag_i, diag_d)) + sub;
            I[j] = std::min(I[j - 1] + e, std::min(M[j - 1], D[j - 1]) + o + e); // row i, column j-1: already this row's
            D[j] = std::min(up_d + e, std::min(up_m, up_i) + o + e);
            diag_m = up_m;
            diag_i = up_i;
            diag_d = up_d;
        }
    }
    return std::min(M[tlen], std::min(I[tlen], D[tlen]));
}
