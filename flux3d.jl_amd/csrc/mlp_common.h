// What the model units (pointnet.hip, dgcnn.hip) share: the exact-Float32 contraction on the f32 MFMA, the activation and
// BatchNorm epilogue, the v_fma_f32 chains of the narrow and the dense layers, and the walk over the flat parameter buffer.
// include/flux3d_hip.h ("PointNet inference") states the arithmetic; pointnet.hip's header comment the tile and its LDS banks.
#pragma once
#include <cmath>

#include "fx3d_common.h"

namespace fx3d {
namespace mlp {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTile = 64;          // points per block
constexpr int kLd = 130;           // LDS row stride of an activation image of up to 128 channels (floats)
constexpr int kPtThreads = 256;    // 4 waves
constexpr float kBnEps = 1e-5f;    // BatchNorm's default epsilon, 1f-5

struct __attribute__((packed, aligned(4))) W4 { float x, y, z, w; };  // four consecutive weights, 4-byte aligned

struct Bn { const float *g, *b, *m, *v; };
struct Conv { const float *W, *b; Bn bn; };
struct Dense { const float *W, *b; };

enum Epi { kNone, kReluBn, kBnRelu, kBnOnly };

// Julia's max on IEEE floats: NaN propagates, -0.0 < +0.0 (as transforms.hip)
__device__ __forceinline__ float jmax(float x, float y) {
    return ((y > x) || (!signbit(y) && signbit(x))) ? (isnan(x) ? x : y) : (isnan(y) ? y : x);
}
__device__ __forceinline__ float relu(float v) { return jmax(0.0f, v); }  // max(zero(v), v)
__device__ __forceinline__ float batchnorm(float v, float g, float be, float mu, float sd) { return (g * ((v - mu) / sd)) + be; }

template <int EPI>
__device__ __forceinline__ float epilogue(float acc, float bias, float g, float be, float mu, float sd) {
    if (EPI == kNone) return acc;
    float v = acc + bias;
    if (EPI == kReluBn) v = relu(v);
    v = batchnorm(v, g, be, mu, sd);
    if (EPI == kBnRelu) v = relu(v);
    return v;
}

// One slab of 32 output channels for both 32-point halves of the tile: acc[p][o] = the fmaf chain over c < CIN, ascending, from
// +0.0f.  a0 / a1: this lane's row of the two halves (in + j LD + h, and 32 rows on); wrow: this lane's weight row W + CIN o.
template <int CIN>
__device__ __forceinline__ void mfma_slab(const float *a0, const float *a1, const float *__restrict__ wrow, int h, f32x16 &acc0,
                                          f32x16 &acc1) {
#pragma unroll 4
    for (int q = 0; q < CIN / 4; ++q) {
        const W4 w = *reinterpret_cast<const W4 *>(wrow + 4 * q);
        const float b0 = h ? w.y : w.x, b1 = h ? w.w : w.z;  // k = 4q + h, then k = 4q + 2 + h
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[4 * q], b0, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[4 * q], b0, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[4 * q + 2], b1, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[4 * q + 2], b1, acc1, 0, 0, 0);
    }
}

// the accumulator's row r of a lane in half-wave h: the point within its 32-point half
__device__ __forceinline__ int mfma_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// out[p][o] = epilogue(sum_c in[p][c] W[c + CIN o]) for the 64 points of the tile and o < cout (a multiple of 32), on the
// f32 MFMA.  FINAL: nothing is stored; tmax[o] = max over the tile's first `nvalid` points.  All 4 waves call it.
// LD: the row stride of both images (LD mod 64 = 2 keeps the bank pattern of kLd).
template <int CIN, int EPI, bool FINAL, int LD = kLd>
__device__ __forceinline__ void conv_mfma(const float *in, float *out, int cout, const float *__restrict__ W,
                                          const float *__restrict__ bias, const Bn bn, int nvalid, float *__restrict__ tmax) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, j = lane & 31;
    const float *a0 = in + j * LD + h, *a1 = a0 + 32 * LD;
    for (int sl = wave; sl < cout / 32; sl += kPtThreads / 64) {
        const int o = sl * 32 + j;
        f32x16 acc0 = {0}, acc1 = {0};
        mfma_slab<CIN>(a0, a1, W + (size_t)CIN * o, h, acc0, acc1);
        float bi = 0.0f, g = 0.0f, be = 0.0f, mu = 0.0f, sd = 1.0f;
        if (EPI != kNone) {
            bi = bias[o]; g = bn.g[o]; be = bn.b[o]; mu = bn.m[o];
            sd = sqrtf(bn.v[o] + kBnEps);
        }
        float m = __int_as_float(0xff800000);  // -Inf: neutral for Julia's max
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int p = mfma_row(r, h);
            const float v0 = epilogue<EPI>(acc0[r], bi, g, be, mu, sd), v1 = epilogue<EPI>(acc1[r], bi, g, be, mu, sd);
            if (FINAL) {
                if (p < nvalid) m = jmax(m, v0);
                if (p + 32 < nvalid) m = jmax(m, v1);
            } else {
                out[p * LD + o] = v0;
                out[(p + 32) * LD + o] = v1;
            }
        }
        if (FINAL) {
            m = jmax(m, __shfl_xor(m, 32, 64));
            if (h == 0) tmax[o] = m;
        }
    }
}

// the same for 3 input channels held as xs[p][3], cout <= 64: one v_fma_f32 chain per (point, channel)
template <int EPI>
__device__ __forceinline__ void conv3(const float *xs, float *out, int ld, int cout, const float *__restrict__ W,
                                      const float *__restrict__ bias, const Bn bn) {
    for (int idx = threadIdx.x; idx < kTile * cout; idx += kPtThreads) {
        const int p = idx / cout, o = idx - p * cout;
        float acc = 0.0f;
        acc = fmaf(xs[p * 3 + 0], W[3 * o + 0], acc);
        acc = fmaf(xs[p * 3 + 1], W[3 * o + 1], acc);
        acc = fmaf(xs[p * 3 + 2], W[3 * o + 2], acc);
        if (EPI == kNone) out[p * ld + o] = acc;
        else out[p * ld + o] = epilogue<EPI>(acc, bias[o], bn.g[o], bn.b[o], bn.m[o], sqrtf(bn.v[o] + kBnEps));
    }
}

// x[0 .. n) in LDS, W (nout, n) column-major: acc = fmaf(x[i], W[o, i], acc) upwards from +0.0f
__device__ __forceinline__ float dense_chain(const float *x, int n, const float *__restrict__ W, int nout, int o) {
    float acc = 0.0f;
    const float *w = W + o;
#pragma unroll 8
    for (int i = 0; i < n; ++i) acc = fmaf(x[i], w[(size_t)nout * i], acc);
    return acc;
}

// ---- the flat parameter buffer, layer by layer in forward order (flux3d_hip.h) ------------------------------------------
struct Cursor {
    const float *base;
    long long at;
    const float *take(long long n) {
        const float *p = base ? base + at : nullptr;
        at += n;
        return p;
    }
    Conv conv(int cin, int cout) {
        Conv c{};
        c.W = take((long long)cin * cout);
        c.b = take(cout);
        return c;
    }
    Bn bn(int c) {
        Bn r;
        r.g = take(c); r.b = take(c); r.m = take(c); r.v = take(c);
        return r;
    }
    Dense dense(int in, int out) {
        Dense d;
        d.W = take((long long)in * out);
        d.b = take(out);
        return d;
    }
};

}  // namespace mlp
}  // namespace fx3d
