/* The contraction of tests/pointnet_ref.py with libm's fmaf: out[p][o] = the chain acc = fmaf(x[p][c], W[c][o], acc) over
 * c ascending from +0.0f.  x (P, cin), W (cin, cout), out (P, cout), all row-major.  Compiled by the test that uses it. */
#include <math.h>
#include <stdint.h>

void pointnet_ref_contract(const float *x, int64_t P, int32_t cin, const float *W, int32_t cout, float *out) {
#pragma omp parallel for schedule(static)
    for (int64_t p = 0; p < P; ++p) {
        float *acc = out + p * cout;
        for (int32_t o = 0; o < cout; ++o) acc[o] = 0.0f;
        for (int32_t c = 0; c < cin; ++c) {
            const float xc = x[p * cin + c];
            const float *w = W + (int64_t)c * cout;
            for (int32_t o = 0; o < cout; ++o) acc[o] = fmaf(xc, w[o], acc[o]);
        }
    }
}
