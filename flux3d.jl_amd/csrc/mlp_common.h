// What the model units (pointnet.hip and pointnet_grad.hip through pointnet_net.h, dgcnn.hip, edgeconv.hip, and through edgeconv_adjoint.h edgeconv_bwd.hip and
// edgeconv_pgrad.hip) share: the exact-Float32 contraction on the f32 MFMA, the
// activation and BatchNorm epilogue, the v_fma_f32 chains of the narrow and the dense layers, the EdgeConv kernel's gather of
// the edge rows and fold of the last layer, the two ends of a classifier head, and on the host the walk over the flat
// parameter buffer, the workspace allocator, the size limits of the neighbour search, the EdgeConv envelope, LDS budget and row stride, and the EdgeConv entry DGCNN and the adjoints run on.
// What only the adjoints share is in edgeconv_adjoint.h.
// What the EdgeConv forward and its training-mode forward share -- the kernel's arguments and its loop over k -- is in edgeconv_net.h.
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
constexpr int kFeat = 1024;        // channels of the pooled feature
constexpr int kHeadThreads = 1024; // a head block: one thread per pooled channel
constexpr float kBnEps = 1e-5f;    // BatchNorm's default epsilon, 1f-5

// The EdgeConv kernels' (edgeconv.hip and the adjoints) dynamic LDS, at most two 64-row images of the widest stride: 132 KB of the
// CU's 160 KB.  Their images share one row stride, the smallest of 66 / kLd / 258 that holds the widest row they keep.
constexpr size_t kMaxLds = (size_t)2 * kTile * 258 * sizeof(float);
inline int edge_stride(int widest) { return widest <= 64 ? 66 : widest <= 128 ? kLd : 258; }

struct __attribute__((packed, aligned(4))) W4 { float x, y, z, w; };  // four consecutive weights, 4-byte aligned

struct Bn { const float *g, *b, *m, *v; };
struct Conv { const float *W, *b; Bn bn; };
struct Dense { const float *W, *b; };

enum Epi { kNone, kReluBn, kBnRelu, kBnOnly, kRelu };  // kRelu: relu(acc + bias), what kReluBn hands its BatchNorm (the adjoints)

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
    if (EPI == kRelu) return relu(v);
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

// mfma_slab for a width known at run time only, on NH = 2 or 1 of the image's 32-point halves; `in`: row 0 of the first of
// them, row stride LD (a constant: every LDS address of the lane is one register plus an immediate offset); j, h: the lane
// within its half-wave and the half-wave.  The MFMA walks the first 4 floor(cin / 4) channels; the same chain then goes on,
// channel by channel, as v_fma_f32 on the accumulator's elements (the rows of mfma_row): cin needs no padding, and a
// contraction is never padded with zero channels (0 * Inf is NaN; pointnet.hip's header comment).  cin < 4 is v_fma_f32 alone.
template <int LD, int NH>
__device__ __forceinline__ void mfma_slab_rt(const float *in, const float *__restrict__ wrow, int cin, int h, int j,
                                             f32x16 (&acc)[NH]) {
    const float *a = in + j * LD + h;
    const int c4 = cin & ~3;
#pragma unroll 4
    for (int c = 0; c < c4; c += 4) {
        const W4 w = *reinterpret_cast<const W4 *>(wrow + c);
        const float b0 = h ? w.y : w.x, b1 = h ? w.w : w.z;
#pragma unroll
        for (int t = 0; t < NH; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t * 32 * LD + c], b0, acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < NH; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t * 32 * LD + c + 2], b1, acc[t], 0, 0, 0);
    }
    const float *t0 = in + 4 * h * LD;  // row mfma_row(r, h) is 4 h + mfma_row(r, 0)
#pragma unroll 1
    for (int c = c4; c < cin; ++c) {
        const float w = wrow[c];
#pragma unroll
        for (int r = 0; r < 16; ++r)
#pragma unroll
            for (int t = 0; t < NH; ++t) acc[t][r] = fmaf(t0[(t * 32 + mfma_row(r, 0)) * LD + c], w, acc[t][r]);
    }
}

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

// ---- the EdgeConv kernel's (edgeconv.hip) gather and fold ---------------------------------------------------------------
// The edge rows [x_n (F), x_idx(k,n) - x_n (F)] of the tile's 64 points in `rows` (row stride ld).  xb: the cloud (F, N);
// ib: the neighbour lists of the tile's points (K each); p0: the tile's first point.  gather_centre writes the x_n half, which
// does not depend on k; gather_diff the other half for rank k, one Float32 subtraction from the x_n the row holds.  A thread
// owns the same (point, channel) pairs in both: element i = p F + c for i = tid, tid + 256, ...  F is known at run time only:
// p comes from one Float32 multiplication, exact for i < 2^13 and F <= 128 ((i + 1/2) / F is at least 1 / 256 away from every
// integer, the product's error below 1e-5).  An index outside [0, N) reads the point itself; rows beyond the cloud's last
// point are zeros.
__device__ __forceinline__ int edge_row_of(int i, float rf) { return (int)(((float)i + 0.5f) * rf); }
__device__ __forceinline__ void gather_centre(float *rows, int ld, const float *xb, int F, int p0, int nvalid) {
    const float rf = 1.0f / (float)F;
    for (int i = threadIdx.x; i < kTile * F; i += kPtThreads) {
        const int p = edge_row_of(i, rf), c = i - p * F;
        rows[p * ld + c] = p < nvalid ? xb[(size_t)(p0 + p) * F + c] : 0.0f;
    }
}
__device__ __forceinline__ void gather_diff(float *rows, int ld, const float *xb, const int32_t *ib, int F, int N, int K, int k,
                                            int p0, int nvalid) {
    const float rf = 1.0f / (float)F;
    for (int i = threadIdx.x; i < kTile * F; i += kPtThreads) {
        const int p = edge_row_of(i, rf), c = i - p * F;
        float *row = rows + p * ld;
        float v = 0.0f;
        if (p < nvalid) {
            int jn = ib[(size_t)p * K + k];
            jn = (unsigned int)jn < (unsigned int)N ? jn : p0 + p;  // (the search returns valid indices only)
            v = xb[(size_t)jn * F + c] - row[c];
        }
        row[F + c] = v;
    }
}

// The last layer of an EdgeConv, never stored: its slab of channel o for the current k folded into the running Julia max per
// (point, channel) that the lane keeps in registers: rm[r] = jmax(rm[r], relu(BN(acc[r] + b))).  fold_half: one 32-point half.
__device__ __forceinline__ void fold_half(const f32x16 &acc, const Conv &c, int o, f32x16 &rm) {
    const float bi = c.b[o], g = c.bn.g[o], be = c.bn.b[o], mu = c.bn.m[o], sd = sqrtf(c.bn.v[o] + kBnEps);
#pragma unroll
    for (int r = 0; r < 16; ++r) rm[r] = jmax(rm[r], epilogue<kBnRelu>(acc[r], bi, g, be, mu, sd));
}
__device__ __forceinline__ void fold_slab(const f32x16 &acc0, const f32x16 &acc1, const Conv &c, int o, f32x16 &rm0, f32x16 &rm1) {
    const float bi = c.b[o], g = c.bn.g[o], be = c.bn.b[o], mu = c.bn.m[o], sd = sqrtf(c.bn.v[o] + kBnEps);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        rm0[r] = jmax(rm0[r], epilogue<kBnRelu>(acc0[r], bi, g, be, mu, sd));
        rm1[r] = jmax(rm1[r], epilogue<kBnRelu>(acc1[r], bi, g, be, mu, sd));
    }
}
template <int NS>
__device__ __forceinline__ void fold_init(f32x16 (&rm0)[NS], f32x16 (&rm1)[NS]) {
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int r = 0; r < 16; ++r) rm0[s][r] = rm1[s][r] = __int_as_float(0xff800000);  // -Inf: neutral for Julia's max
}
// After the last k: the tile's (cout, 64) part of the (cout, N, B) output with plain stores.  A wave owns the slabs wave,
// wave + 4, ... of 32 channels (NS of them at most); ob: the output row of the tile's first point.
template <int NS>
__device__ __forceinline__ void fold_store(float *ob, int cout, int nvalid, const f32x16 (&rm0)[NS], const f32x16 (&rm1)[NS]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, j = lane & 31;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int o = (wave + s * (kPtThreads / 64)) * 32 + j;
        if (o - j >= cout) break;  // wave-uniform
        if (o >= cout) continue;   // the lanes beyond a partial slab
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int p = mfma_row(r, h);
            if (p < nvalid) ob[(size_t)p * cout + o] = rm0[s][r];
            if (p + 32 < nvalid) ob[(size_t)(p + 32) * cout + o] = rm1[s][r];
        }
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

// dz[0 .. nout) in LDS, W (nout, nin) column-major, nout a multiple of 4: acc = fmaf(dz[o], W[o, i], acc) upwards from +0.0f
__device__ __forceinline__ float transposed_chain(const float *dz, int nout, const float *__restrict__ W, int i) {
    float acc = 0.0f;
    const float *w = W + (size_t)nout * i;
#pragma unroll 4
    for (int o = 0; o < nout; o += 4) {
        const W4 q = *reinterpret_cast<const W4 *>(w + o);
        acc = fmaf(dz[o], q.x, acc);
        acc = fmaf(dz[o + 1], q.y, acc);
        acc = fmaf(dz[o + 2], q.z, acc);
        acc = fmaf(dz[o + 3], q.w, acc);
    }
    return acc;
}

// The parameter sums of a dense layer over the clouds (the adjoints' dense_sums_kernel): H[o, i] = the chain over b of
// d[o, b] a[i, b], h[o] = the sum over b of d[o, b]; element e of nin nout + nout, one thread each
struct DenseSums { const float *d, *a; int nin, nout, B; float *H, *h; };
__device__ __forceinline__ void dense_sums(const DenseSums &s, long long e) {
    const long long nw = (long long)s.nin * s.nout;
    if (e < nw) {
        const int i = (int)(e / s.nout), o = (int)(e - (long long)i * s.nout);
        float acc = 0.0f;
#pragma unroll 8
        for (int b = 0; b < s.B; ++b) acc = fmaf(s.d[o + (size_t)s.nout * b], s.a[i + (size_t)s.nin * b], acc);
        s.H[e] = acc;
    } else if (e < nw + s.nout) {
        const int o = (int)(e - nw);
        float acc = 0.0f;
        for (int b = 0; b < s.B; ++b) acc = acc + s.d[o + (size_t)s.nout * b];
        s.h[o] = acc;
    }
}

// ---- the two ends of a head kernel (one block of kHeadThreads per cloud b) -------------------------------------------------
// MaxPool over the cloud's points: thread tid folds channel tid of the per-tile maxima tmax (kFeat, ntiles, B)
__device__ __forceinline__ float fold_tile_maxima(const float *tmax, int ntiles, int b) {
    const float *t = tmax + (size_t)b * ntiles * kFeat + threadIdx.x;
    float m = t[0];
    for (int k = 1; k < ntiles; ++k) m = jmax(m, t[(size_t)k * kFeat]);
    return m;
}
// pr = softmax(z) over the n logits the block has just written to z (both in memory): the maximum and the sum in class
// order, each in thread 0
__device__ __forceinline__ void softmax_of_logits(const float *z, float *pr, int n) {
    __shared__ float zmax, esum;
    const int tid = threadIdx.x;
    __syncthreads();  // the block's logits are in memory
    if (tid == 0) {
        float m = z[0];
        for (int i = 1; i < n; ++i) m = jmax(m, z[i]);
        zmax = m;
    }
    __syncthreads();
    for (int o = tid; o < n; o += kHeadThreads) pr[o] = expf(z[o] - zmax);
    __syncthreads();
    if (tid == 0) {
        float s = 0.0f;
        for (int i = 0; i < n; ++i) s = s + pr[i];  // in class order
        esum = s;
    }
    __syncthreads();
    for (int o = tid; o < n; o += kHeadThreads) pr[o] = pr[o] / esum;
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

// ---- the sizes an EdgeConv takes (dgcnn.hip, edgeconv.hip), for the entry point `fn` ----------------------------------------
constexpr int kMaxN = 36864;  // the neighbour search's general kernel holds a query's N distance keys in LDS
inline fx3d_status check_edgeconv_sizes(const char *fn, int32_t N, int32_t B, int32_t K) {
    FX3D_REQUIRE(N >= 1 && B >= 1, "%s: N and B must be positive, got N=%d B=%d", fn, N, B);
    FX3D_REQUIRE(K >= 1, "%s: K must be positive, got %d", fn, K);
    FX3D_REQUIRE((long long)K + 1 <= N, "%s: K + 1 = %lld neighbours (the point itself is dropped) of N = %d points", fn, (long long)K + 1, N);
    FX3D_REQUIRE(N <= kMaxN, "%s: N must be at most %d (the neighbour search), got %d", fn, kMaxN, N);
    FX3D_REQUIRE(B <= 65535, "%s: B must be at most 65535, got %d", fn, B);
    FX3D_REQUIRE((long long)N * B * K <= (1ll << 31), "%s: N * B * K must be at most 2^31, got %lld", fn, (long long)N * B * K);
    return FX3D_OK;
}

// the envelope of an EdgeConv (edgeconv.hip, edgeconv_bwd.hip, edgeconv_pgrad.hip), for the entry point `fn`
constexpr int kMaxLayers = 4;     // conv_bn_blocks of one EdgeConv
constexpr int kMaxF = 128;        // input features: an edge row has 2 F channels, one image row of stride 258 at most
constexpr int kMaxWidth = 256;    // 8 slabs of 32 channels = 2 per wave = 64 VGPRs of running maxima per lane
inline fx3d_status check_layers(const char *fn, const int32_t *layers, int32_t nlayers) {
    FX3D_REQUIRE(layers != nullptr, "%s: layers is NULL", fn);
    if (nlayers < 2 || nlayers > kMaxLayers + 1) {
        set_error("%s: layers must hold F and 1 to %d widths, got %d entries", fn, kMaxLayers, nlayers);
        return FX3D_ERR_UNSUPPORTED;
    }
    if (layers[0] < 1 || layers[0] > kMaxF) {
        set_error("%s: layers[0] = F must be in [1, %d] (an edge row has 2 F channels), got %d", fn, kMaxF, layers[0]);
        return FX3D_ERR_UNSUPPORTED;
    }
    for (int i = 1; i < nlayers; ++i)
        if (layers[i] < 1 || layers[i] > kMaxWidth) {
            set_error("%s: layers[%d] must be in [1, %d], got %d", fn, i, kMaxWidth, layers[i]);
            return FX3D_ERR_UNSUPPORTED;
        }
    return FX3D_OK;
}

// ---- edgeconv.hip: EdgeConv(layers, K) on x (F, N, B) -> out (cL, N, B), for fx3d_edgeconv_forward and fx3d_dgcnn_forward -----
// The arguments are fx3d_edgeconv_forward's (flux3d_hip.h), already checked: layers by the envelope, N, B, K by
// check_edgeconv_sizes, ws 256-byte aligned and of edgeconv_workspace_bytes(F = layers[0], ...) at least.  `label`: the name
// of the kernel's launches in the library's profile.  edgeconv_layout: the length of the parameter buffer in floats (and, with
// c, its layers).
long long edgeconv_layout(const float *params, const int32_t *layers, int nlayers, Conv *c);
fx3d_status edgeconv_workspace_bytes(int F, int N, int B, int K, size_t *bytes);
fx3d_status edgeconv_run(const float *params_dev, const int32_t *layers, int nlayers, int K, const float *x, int N, int B,
                         const int32_t *idx_in, float *out, int32_t *idx_out, void *ws, fx3d_stream_t s, const char *label);


}  // namespace mlp
}  // namespace fx3d
