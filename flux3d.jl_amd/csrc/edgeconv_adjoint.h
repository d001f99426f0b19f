// What the two EdgeConv adjoints (edgeconv_bwd.hip: the input adjoint; edgeconv_pgrad.hip: the parameter adjoint, which also
// returns gx) share: the chain per neighbour rank k, step by step, the kernel arguments of the chain, and on the host the
// workspace prefix and everything an entry point does between its NULL check and its launch.  Both kernels call the steps below
// in the order of their header comments, so the two compute gx with the same instructions in the same order.
// The training-mode adjoint (edgeconv_grad_train.hip) calls the same steps in their training mode (TrainBn below), its closing pass
// through the parameter adjoint's kernel (edgeconv_pgrad_net.h).
//
// A tile is 32 NH points of one cloud in LDS images of row stride LD; a lane owns one channel (j of the wave's slab of 32) and
// the 16 rows mfma_row(r, h) of each 32-point half; wave w owns the slabs w, w + 4, ... of every layer, NS of them at most of the
// last layer and of the 2F.  A step that hands registers on takes a sink, sink(sl, d): the wave's slab sl as it stands in the
// accumulators' rows.  The input adjoint has no use for them (NoSink); the parameter adjoint contracts them.
//
// Not here: the target load before a tile's first k (tgt, the upstream values, dz0), which each kernel keeps in its body.  As a
// shared step it left edgeconv_pgrad_kernel<258, 2, 12>, which sits at 256 + 252 registers, with scratch in every form tried.
#pragma once
#include "mlp_common.h"

namespace fx3d {
namespace mlp {

constexpr int kWaves = kPtThreads / 64;

struct AdjointArgs {
    const float *x;      // (F, N, B)
    const int32_t *idx;  // (K, N, B), 0-based
    const float *out;    // (cL, N, B): the forward's
    const float *gout;   // (cL, N, B)
    float *gx;           // (F, N, B); the parameter adjoint: or NULL
    Conv c[kMaxLayers];
    const float *wt[kMaxLayers];  // Wt_l[o + cout c]
    int w[kMaxLayers + 1];        // F, c1, ..., cL
    int nl, cout;                 // L, cL
    int N, K;
};

struct NoSink {  // for last_compare's sink(sl, d) and back_layer's sink(l, sl, d)
    template <class... A>
    __device__ __forceinline__ void operator()(const A &...) const {}
};

__device__ __forceinline__ float quiet_nan() { return __int_as_float(0x7fc00000); }

// The mode of the steps that cross a BatchNorm (last_compare, hidden_bwd, back_layer).  EvalBn: test mode, mu and var constants, what
// goes below a BatchNorm is (d gamma) / sd row by row.  TrainBn ("EdgeConv training-mode adjoint", edgeconv_grad_train.hip): the
// BatchNorms at the batch statistics (the caller puts them where a.c[].bn.m / .v point), every BatchNorm a cut:
//   gy = the gradient at the BatchNorm's output (gout where chosen; below, d where the relu let through), xh = ((z + b) - mu) / sd of
//   EVERY row, the forward's bits: of layer L from the compare's accumulators, of a hidden layer from one more forward slab on the
//   image below it, which the parameter adjoint's LDS plan keeps (the lane that owns channel c of d owns c of the slab, same rows);
//   gv = (((gy - mb) - (xh mg)) gamma) / sd takes dz's place, +0 in the rows beyond the cloud's last point;
//   means: Float32(dbeta64 / m), then Float32(dgamma64 / m) per layer, in the statistics buffer's layout, finished for the layers
//   above `stop`; stop: the layer whose (gy, gy xh) sums this pass takes -- the walk ends there and nothing is written for it --
//   or 0: the closing pass.
// A training-mode sink is sink(sl, gy, xh, gv): at the stop layer gy and xh as they enter the sums (+0 in the rows that add
// nothing: beyond the cloud, and at layer L every row but the chosen one), gv elsewhere.  Only the images of edgeconv_pgrad.hip's
// plan (32 rows, image l - 2 alive while layer l walks back) serve this mode.
struct EvalBn {
    static constexpr bool kTrain = false;
};
struct TrainBn {
    static constexpr bool kTrain = true;
    const float *means;
    int stop, nvalid;
};
// where layer l's (1-based) block of a buffer in the statistics layout begins: 2 (c1 + .. + c_{l-1})
__device__ __forceinline__ int stat_offset(const int (&w)[kMaxLayers + 1], int l) {
    return 2 * ((l > 1 ? w[1] : 0) + (l > 2 ? w[2] : 0) + (l > 3 ? w[3] : 0));
}
// gv of one element; valid: the row is one of the cloud's
__device__ __forceinline__ float train_gv(float gy, float xh, float mb, float mg, float g, float sd, bool valid) {
    float t = gy - mb;
    t = t - (xh * mg);
    return valid ? (t * g) / sd : 0.0f;
}

// gather_centre and gather_diff in one pass, for a tile of T points: both halves are written with every k
template <int T>
__device__ __forceinline__ void gather_rows(float *rows, int ld, const float *xb, const int32_t *ib, int F, int N, int K, int k,
                                            int p0, int nvalid) {
    const float rf = 1.0f / (float)F;
    for (int i = threadIdx.x; i < T * F; i += kPtThreads) {
        const int p = edge_row_of(i, rf), c = i - p * F;
        float xc = 0.0f, v = 0.0f;
        if (p < nvalid) {
            xc = xb[(size_t)(p0 + p) * F + c];
            int jn = ib[(size_t)p * K + k];
            jn = (unsigned int)jn < (unsigned int)N ? jn : p0 + p;
            v = xb[(size_t)jn * F + c] - xc;
        }
        rows[p * ld + c] = xc;
        rows[p * ld + F + c] = v;
    }
}

// one hidden layer forward, image to image: conv_item of edgeconv.hip on the wave's slabs
template <int LD, int NH>
__device__ __forceinline__ void hidden_fwd(const float *in, float *out, int cin, int cout, const Conv &c) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, j = lane & 31;
    for (int sl = wave; sl * 32 < cout; sl += kWaves) {
        const int o = sl * 32 + j, oc = min(o, cout - 1);
        f32x16 acc[NH];
#pragma unroll
        for (int t = 0; t < NH; ++t) acc[t] = f32x16{0};
        mfma_slab_rt<LD, NH>(in, c.W + (size_t)cin * oc, cin, h, j, acc);
        const float bi = c.b[oc], g = c.bn.g[oc], be = c.bn.b[oc], mu = c.bn.m[oc], sd = sqrtf(c.bn.v[oc] + kBnEps);
        if (o < cout) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
#pragma unroll
                for (int t = 0; t < NH; ++t) out[(t * 32 + mfma_row(r, h)) * LD + o] = epilogue<kBnRelu>(acc[t][r], bi, g, be, mu, sd);
        }
    }
}

// The hidden layers forward, from the edge rows in img[0] through img[1 .. L-1] (a barrier after each): the last layer's source
// image (its width: the kernels' cinl).  The layers by wave-uniform selects, as edgeconv_kernel.
template <int LD, int NH>
__device__ __forceinline__ const float *hidden_fwd_chain(const AdjointArgs &a, float *lds, int F, int L) {
    constexpr int IMG = 32 * NH * LD;
    const float *src = lds;
    int cin = 2 * F;
    for (int i = 0; i + 1 < L; ++i) {
        const Conv c = i == 0 ? a.c[0] : i == 1 ? a.c[1] : a.c[2];
        const int co = i == 0 ? a.w[1] : i == 1 ? a.w[2] : a.w[3];
        float *dst = lds + (i + 1) * IMG;
        hidden_fwd<LD, NH>(src, dst, cin, co, c);
        __syncthreads();
        src = dst;
        cin = co;
    }
    return src;
}

// The last layer for the current k, slab by slab as edgeconv_kernel computes it (mfma_slab_rt, epilogue<kBnRelu>: the forward's
// bits), compared with tgt (the forward's out where positive, else NaN): dz_L into dzl, tgt retired (NaN) where this k is the
// first to reproduce it -- the first k that equals the maximum takes the gradient, no later one does (NaN == anything is false).
// up: the upstream values.  SCALED (the input adjoint): (gout gamma_L) / sd_L, computed once per tile, is what dz_L is where k is
// chosen.  Else (the parameter adjoint, which needs d_L itself and has no registers for both): gout, scaled here.  dz0:
// (+0 gamma_L) / sd_L, what dz_L is elsewhere.  The sink gets the slab's `up` where chosen, +0 elsewhere: d_L unless SCALED.
// Mode::kTrain: `up` is gout (SCALED and dz0 have no part), moff: layer L's stat_offset; stopped: L is the stop layer (else gv_L into dzl).
template <int LD, int NH, int NS, bool SCALED, class Sink, class Mode = EvalBn>
__device__ __forceinline__ void last_compare(const float *src, float *dzl, const Conv &cl, int cinl, int cout, int wave, int h, int j,
                                             f32x16 (&tgt)[NS][NH], const f32x16 (&up)[NS][NH], const float (&dz0)[NS], Sink &&sink,
                                             const Mode &m = Mode{}, int moff = 0, bool stopped = false) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int sl = wave + s * kWaves;
        if (sl * 32 >= cout) continue;  // wave-uniform
        const int o = sl * 32 + j, oc = min(o, cout - 1);
        f32x16 acc[NH], d[NH];
#pragma unroll
        for (int t = 0; t < NH; ++t) acc[t] = f32x16{0};
        mfma_slab_rt<LD, NH>(src, cl.W + (size_t)cinl * oc, cinl, h, j, acc);
        const float bi = cl.b[oc], g = cl.bn.g[oc], be = cl.bn.b[oc], mu = cl.bn.m[oc], sd = sqrtf(cl.bn.v[oc] + kBnEps);
        if constexpr (Mode::kTrain) {
            const bool stop = stopped;
            float mb = 0.0f, mg = 0.0f;
            if (!stop) {
                mb = m.means[moff + oc];
                mg = m.means[moff + cout + oc];
            }
            f32x16 xs[NH], gv[NH];
#pragma unroll
            for (int r = 0; r < 16; ++r)
#pragma unroll
                for (int t = 0; t < NH; ++t) {
                    const float xh = ((acc[t][r] + bi) - mu) / sd;  // epilogue<kBnRelu>'s own operations, xh kept
                    const bool first = relu((g * xh) + be) == tgt[s][t][r];
                    const float gy = first ? up[s][t][r] : 0.0f;
                    tgt[s][t][r] = first ? quiet_nan() : tgt[s][t][r];
                    d[t][r] = gy;
                    xs[t][r] = first ? xh : 0.0f;
                    gv[t][r] = 0.0f;
                    if (!stop) {
                        gv[t][r] = train_gv(gy, xh, mb, mg, g, sd, t * 32 + mfma_row(r, h) < m.nvalid);
                        if (o < cout) dzl[(t * 32 + mfma_row(r, h)) * LD + o] = gv[t][r];
                    }
                }
            sink(sl, d, xs, gv);
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r)
#pragma unroll
                for (int t = 0; t < NH; ++t) {
                    const bool first = epilogue<kBnRelu>(acc[t][r], bi, g, be, mu, sd) == tgt[s][t][r];
                    const float u = up[s][t][r];
                    if (o < cout) dzl[(t * 32 + mfma_row(r, h)) * LD + o] = first ? (SCALED ? u : (u * g) / sd) : dz0[s];
                    d[t][r] = first ? u : 0.0f;
                    tgt[s][t][r] = first ? quiet_nan() : tgt[s][t][r];
                }
            sink(sl, d);
        }
    }
}

// one hidden layer backward: d[p][c] = the chain over o < cout of dz[p][o] Wt[o + cout c] for c < cin, then in a's place
// dz'[p][c] = ((a[p][c] > 0 ? d : +0) gamma[c]) / sd[c] with the BatchNorm of the layer that made a
// sink(sl, d): d before gamma and sd; what the lanes beyond cin hold there is not d.
// Mode::kTrain: fw, ain, cprev: the convolution that made a, its input image and width, for xh; moff: its layer's stat_offset;
// stopped: it is the stop layer (a stays as it is).
template <int LD, int NH, class Sink, class Mode = EvalBn>
__device__ __forceinline__ void hidden_bwd(const float *dz, float *a, int cout, int cin, const float *__restrict__ wt, const Bn &bn,
                                           Sink &&sink, const Mode &m = Mode{}, const Conv *fw = nullptr, const float *ain = nullptr,
                                           int cprev = 0, int moff = 0, bool stopped = false) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, j = lane & 31;
    for (int sl = wave; sl * 32 < cin; sl += kWaves) {
        const int c = sl * 32 + j, cc = min(c, cin - 1);
        f32x16 acc[NH];
#pragma unroll
        for (int t = 0; t < NH; ++t) acc[t] = f32x16{0};
        mfma_slab_rt<LD, NH>(dz, wt + (size_t)cout * cc, cout, h, j, acc);
        const float g = bn.g[cc], sd = sqrtf(bn.v[cc] + kBnEps);
        if constexpr (Mode::kTrain) {
            f32x16 v[NH], xs[NH], gv[NH];
#pragma unroll
            for (int t = 0; t < NH; ++t) v[t] = xs[t] = gv[t] = f32x16{0};
            mfma_slab_rt<LD, NH>(ain, fw->W + (size_t)cprev * cc, cprev, h, j, v);  // z of the layer that made a: the forward's slab
            const float bi = fw->b[cc], mu = bn.m[cc];
            float mb = 0.0f, mg = 0.0f;
            if (!stopped) {
                mb = m.means[moff + cc];
                mg = m.means[moff + cin + cc];
            }
#pragma unroll
            for (int r = 0; r < 16; ++r)
#pragma unroll
                for (int t = 0; t < NH; ++t) {
                    float *e = a + (t * 32 + mfma_row(r, h)) * LD + c;
                    const bool valid = t * 32 + mfma_row(r, h) < m.nvalid;
                    const float al = c < cin ? *e : 0.0f;
                    const float gy = al > 0.0f ? acc[t][r] : 0.0f;
                    const float xh = ((v[t][r] + bi) - mu) / sd;
                    acc[t][r] = valid ? gy : 0.0f;
                    xs[t][r] = valid ? xh : 0.0f;
                    if (!stopped) {
                        gv[t][r] = train_gv(gy, xh, mb, mg, g, sd, valid);
                        if (c < cin) *e = gv[t][r];
                    }
                }
            sink(sl, acc, xs, gv);
        } else {
            if (c < cin) {
#pragma unroll
                for (int r = 0; r < 16; ++r)
#pragma unroll
                    for (int t = 0; t < NH; ++t) {
                        float *e = a + (t * 32 + mfma_row(r, h)) * LD + c;
                        const float d = *e > 0.0f ? acc[t][r] : 0.0f;
                        acc[t][r] = d;
                        *e = (d * g) / sd;
                    }
            }
            sink(sl, acc);
        }
    }
}

// One layer of the way back, l = L .. 2 (the parameter adjoint: down to the lowest layer its pass needs): dz_l in img[l] (dz_L in
// dzl), d_{l-1} over ALL o of dz_l with Wt_l, masked by a_{l-1} > 0, to sink(l, sl, d), then times gamma_{l-1}, divided by
// sd_{l-1}, into a_{l-1}'s place in img[l-1]; then a barrier.  The layer by wave-uniform selects among the kernel arguments,
// which fold where the caller's loop is unrolled (the parameter adjoint's, whose sink needs l as a constant).
// Mode::kTrain: layer l - 1 is cut at its BatchNorm (hidden_bwd); sink(l, sl, gy, xh, gv).
template <int LD, int NH, class Sink, class Mode = EvalBn>
__device__ __forceinline__ void back_layer(const AdjointArgs &a, float *lds, const float *dzl, int L, int l, Sink &&sink,
                                           const Mode &m = Mode{}) {
    constexpr int IMG = 32 * NH * LD;
    const float *dz = l == L ? dzl : lds + l * IMG;
    const int co = l == 2 ? a.w[2] : l == 3 ? a.w[3] : a.w[4];
    const int ci = l == 2 ? a.w[1] : l == 3 ? a.w[2] : a.w[3];
    const float *wt = l == 2 ? a.wt[1] : l == 3 ? a.wt[2] : a.wt[3];
    const Bn bn = l == 2 ? a.c[0].bn : l == 3 ? a.c[1].bn : a.c[2].bn;
    if constexpr (Mode::kTrain) {
        const Conv fw = l == 2 ? a.c[0] : l == 3 ? a.c[1] : a.c[2];
        const int cprev = l == 2 ? 2 * a.w[0] : l == 3 ? a.w[1] : a.w[2];
        hidden_bwd<LD, NH>(dz, lds + (l - 1) * IMG, co, ci, wt, bn,
                           [&](int sl, const f32x16(&gy)[NH], const f32x16(&xh)[NH], const f32x16(&gv)[NH]) { sink(l, sl, gy, xh, gv); },
                           m, &fw, lds + (l - 2) * IMG, cprev, stat_offset(a.w, l - 1), m.stop == l - 1);
    } else {
        hidden_bwd<LD, NH>(dz, lds + (l - 1) * IMG, co, ci, wt, bn, [&](int sl, const f32x16(&d)[NH]) { sink(l, sl, d); });
    }
    __syncthreads();
}

// d_0 from dz_1 (img[1] for every L) and Wt_1, added to the sums over k for the lane's channel of the 2F
template <int LD, int NH, int NS>
__device__ __forceinline__ void add_d0(const AdjointArgs &a, const float *lds, int F, int wave, int h, int j, f32x16 (&S)[NS][NH]) {
    constexpr int IMG = 32 * NH * LD;
    const int F2 = 2 * F;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int sl = wave + s * kWaves;
        if (sl * 32 >= F2) continue;  // wave-uniform
        const int cc = min(sl * 32 + j, F2 - 1);
        f32x16 acc[NH];
#pragma unroll
        for (int t = 0; t < NH; ++t) acc[t] = f32x16{0};
        mfma_slab_rt<LD, NH>(lds + IMG, a.wt[0] + (size_t)a.w[1] * cc, a.w[1], h, j, acc);
#pragma unroll
        for (int r = 0; r < 16; ++r)
#pragma unroll
            for (int t = 0; t < NH; ++t) S[s][t][r] = S[s][t][r] + acc[t][r];
    }
}

// After the last k: S to `rows` (last read before a barrier of the k loop), then gx[f] = S[f] - S[F + f] for the tile's points
// (b, p0: the cloud and the tile's first point)
template <int LD, int NH, int NS>
__device__ __forceinline__ void store_gx(const AdjointArgs &a, float *rows, int b, int p0, int nvalid, int wave, int h, int j,
                                         const f32x16 (&S)[NS][NH]) {
    constexpr int T = 32 * NH;
    const int F = a.w[0];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int c = (wave + s * kWaves) * 32 + j;
        if (c >= 2 * F) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r)
#pragma unroll
            for (int t = 0; t < NH; ++t) rows[(t * 32 + mfma_row(r, h)) * LD + c] = S[s][t][r];
    }
    __syncthreads();
    float *gb = a.gx + ((size_t)b * a.N + p0) * F;
    const float rf = 1.0f / (float)F;
    for (int i = threadIdx.x; i < T * F; i += kPtThreads) {
        const int p = edge_row_of(i, rf), c = i - p * F;
        if (p < nvalid) gb[(size_t)p * F + c] = rows[p * LD + c] - rows[p * LD + F + c];
    }
}

// ---- the host side (defined in edgeconv_bwd.hip) ---------------------------------------------------------------------------
// the LDS row stride of both adjoints: the smallest that holds the widest of 2F, c1 .. cL
inline int adjoint_stride(const int32_t *layers, int nlayers) {
    int widest = 2 * layers[0];
    for (int i = 1; i < nlayers; ++i) widest = layers[i] > widest ? layers[i] : widest;
    return edge_stride(widest);
}

// The weights as the adjoints read them, Wt_l[o + cout c] = W_l[c + cin o].  c: edgeconv_layout's layers.  One launch on st
// writes every layer's Wt into wt (edgeconv_transposed_floats floats), wt_of[l] is where layer l + 1's begins.
size_t edgeconv_transposed_floats(const int32_t *layers, int nlayers);
fx3d_status edgeconv_transpose_weights(const Conv *c, const int32_t *layers, int nlayers, float *wt, const float **wt_of, hipStream_t st);

// The workspace prefix of both adjoints, put into ws: the forward's own (the search's scratch) | the neighbour lists (K, N, B) |
// out (cL, N, B) | the transposed weights.  The parameter adjoint appends to the same ws.  First the checks every adjoint entry
// `fn` makes of its sizes: check_layers, check_edgeconv_sizes, the forward's own.
struct AdjointWs { size_t fwd, fwd_bytes, idx, out, wt; };
fx3d_status edgeconv_adjoint_plan(const char *fn, const int32_t *layers, int nlayers, int N, int B, int K, WsBump &ws, AdjointWs *w);

// What an adjoint entry `fn` does between its plan (w; need: its whole workspace, what `size_fn` reports) and its launch: the
// size and alignment refusals, the chain's arguments a from the entry's own, the forward and / or the search where the caller
// gives no out / idx (edgeconv_run and fx3d_knn_ws, as fx3d_edgeconv_forward runs them: the search is deterministic), and the
// transposed weights.  stats (the training-mode adjoint): the batch statistics, in the layout of "DGCNN / EdgeConv training-mode
// forward"; the chain's BatchNorms then read their mean and variance there, and so does the forward where the caller gives no out.
fx3d_status edgeconv_adjoint_prepare(const char *fn, const char *size_fn, const AdjointWs &w, size_t need, const float *params_dev,
                                     const int32_t *layers, int nlayers, int K, const float *x, int N, int B, const int32_t *idx,
                                     const float *out, const float *gout, float *gx, void *ws, size_t ws_bytes, fx3d_stream_t s,
                                     AdjointArgs *a, const float *stats = nullptr);

}  // namespace mlp
}  // namespace fx3d
