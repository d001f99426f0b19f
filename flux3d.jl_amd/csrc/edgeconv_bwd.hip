// EdgeConv(layers, K): the gradient with respect to the input x, test-mode BatchNorm, in one fused kernel (gfx950).
// include/flux3d_hip.h ("EdgeConv input adjoint") states the definition; tests/edgeconv_bwd_ref.py restates it on the host.
// The neighbours are constants (CreateSingleKNNGraph is @nograd), so the gradient of point n depends on the K edge rows of
// point n alone: no scatter, no inverse lists, no atomics.  The arithmetic is the forward's contract (mlp_common.h), transposed.
// The chain's steps are edgeconv_adjoint.h's, which the parameter adjoint (edgeconv_pgrad.hip) calls too; this file owns the
// transpose and the host preamble of both (edgeconv_adjoint_plan, edgeconv_adjoint_prepare).
//
// Per call: the search and / or the forward if the caller does not give idx / out (edgeconv_run and fx3d_knn_ws, as
// fx3d_edgeconv_forward runs them), transpose_weights (Wt_l[o + cout c] = W_l[c + cin o] for every layer into the workspace, so
// that the backward contraction over o reads a lane's weights as one row, which is what mfma_slab_rt takes), then
// edgeconv_bwd_kernel<LD, NH, NS>: one block = 32 NH points of one cloud, 4 waves, looping over the neighbour rank k.
//   LDS: max(L, 2) images of 32 NH rows and one row stride LD = 66 / 130 / 258, the smallest that holds the widest of 2F, c1 .. cL.
//     img[0] = `rows`: the edge rows, then dz_L (L >= 2), after the last k the sums S.  img[l], 1 <= l < L: a_l, overwritten in
//     place by dz_l on the way back (the lane that produces an element is the only one that reads its a_l).  L = 1: dz_1 in img[1].
//     64 points (NH = 2) where that fits 132 KB, else 32 (NH = 1): four images of stride 258 are 132 KB at 32 points.
//   Registers, per lane (one channel, 16 points per 32-point half, NS slabs per wave as in the forward's fold: the strides 66
//   and 130 hold 128 channels = one slab per wave at most, the stride 258 two):
//     tgt  the forward's out where it is positive, else NaN -- and NaN from the k on that reproduced it: the first k that equals
//          the maximum takes the gradient, no later one does ("already chosen" is the NaN; NaN == anything is false);
//     dzg  (gout gamma_L) / sd_L, what dz_L is where k is chosen;  dz0 = (+0 gamma_L) / sd_L, what it is elsewhere;
//     S    the running sums over k of d_0, for the lane's channel of the 2F.
//   Per k (the steps of edgeconv_adjoint.h): gather_rows; hidden_fwd_chain, the hidden layers image to image, and last_compare,
//     the last layer slab by slab, exactly as edgeconv_kernel computes them (mfma_slab_rt, epilogue<kBnRelu>: the forward's bits),
//     compared with tgt, dz_L written; back_layer for l = L .. 2: d_{l-1} = the chain over ALL o of dz_l with Wt_l, masked by
//     a_{l-1} > 0, times gamma_{l-1}, divided by sd_{l-1} into a_{l-1}'s place; add_d0: d_0 from dz_1 and Wt_1, added to S.
//     After the last k, store_gx: S to `rows`, gx[f] = S[f] - S[F + f].
//   A slab beyond a width's last channel: its lanes read the last channel's parameters, run the wave's MFMAs and write nothing.
//   Rows beyond the cloud's last point are zeros with tgt = NaN: computed, never written.
#include "edgeconv_adjoint.h"
#include "edgeconv_net.h"

using namespace fx3d;
using namespace fx3d::mlp;

namespace {

struct TransposeArgs {
    const float *W[kMaxLayers];
    float *wt[kMaxLayers];
    int cin[kMaxLayers], cout[kMaxLayers];
};

// Wt_l[o + cout c] = W_l[c + cin o]; blockIdx.y: the layer
__global__ __launch_bounds__(256) void transpose_weights(const TransposeArgs t) {
    const int l = blockIdx.y;
    const float *W = l == 0 ? t.W[0] : l == 1 ? t.W[1] : l == 2 ? t.W[2] : t.W[3];
    float *wt = l == 0 ? t.wt[0] : l == 1 ? t.wt[1] : l == 2 ? t.wt[2] : t.wt[3];
    const int cin = l == 0 ? t.cin[0] : l == 1 ? t.cin[1] : l == 2 ? t.cin[2] : t.cin[3];
    const int cout = l == 0 ? t.cout[0] : l == 1 ? t.cout[1] : l == 2 ? t.cout[2] : t.cout[3];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < cin * cout; i += gridDim.x * blockDim.x) {
        const int c = i / cout, o = i - c * cout;
        wt[i] = W[c + cin * o];
    }
}

template <int LD, int NH, int NS>
__global__ __launch_bounds__(kPtThreads) void edgeconv_bwd_kernel(const AdjointArgs a) {
    extern __shared__ float lds[];
    constexpr int T = 32 * NH, IMG = T * LD;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, j = lane & 31;
    const int b = blockIdx.y, p0 = blockIdx.x * T;
    const int nvalid = min(T, a.N - p0);
    const int F = a.w[0], L = a.nl, cout = a.cout;
    const float *xb = a.x + (size_t)b * a.N * F;
    const int32_t *ib = a.idx + ((size_t)b * a.N + p0) * a.K;
    float *rows = lds;
    float *dzl = L == 1 ? lds + IMG : lds;  // where dz_L goes
    // the last layer by wave-uniform selects among the kernel arguments (a constant index in every access, as edgeconv_kernel)
    const Conv cl = L == 1 ? a.c[0] : L == 2 ? a.c[1] : L == 3 ? a.c[2] : a.c[3];
    const int cinl = L == 1 ? 2 * F : L == 2 ? a.w[1] : L == 3 ? a.w[2] : a.w[3];  // its input width

    const float nan = quiet_nan();
    f32x16 tgt[NS][NH], dzg[NS][NH], S[NS][NH];
    float dz0[NS];
    // the target load (each adjoint's own, edgeconv_adjoint.h says why)
    {
        const size_t base = ((size_t)b * a.N + p0) * cout;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int sl = wave + s * kWaves;
            dz0[s] = 0.0f;
#pragma unroll
            for (int t = 0; t < NH; ++t) S[s][t] = tgt[s][t] = dzg[s][t] = f32x16{0};
            if (sl * 32 >= cout) continue;  // wave-uniform
            const int oc = min(sl * 32 + j, cout - 1);
            const float g = cl.bn.g[oc], sd = sqrtf(cl.bn.v[oc] + kBnEps);
            dz0[s] = (0.0f * g) / sd;
#pragma unroll
            for (int r = 0; r < 16; ++r)
#pragma unroll
                for (int t = 0; t < NH; ++t) {
                    const int p = t * 32 + mfma_row(r, h);
                    float ov = nan, gv = 0.0f;
                    if (p < nvalid) {
                        ov = a.out[base + (size_t)p * cout + oc];
                        gv = a.gout[base + (size_t)p * cout + oc];
                    }
                    tgt[s][t][r] = ov > 0.0f ? ov : nan;
                    dzg[s][t][r] = (gv * g) / sd;
                }
        }
    }
    for (int k = 0; k < a.K; ++k) {
        // (`rows` was last read before a barrier of the previous k: by its first layer, or by hidden_bwd of layer L as dz_L)
        gather_rows<T>(rows, LD, xb, ib, F, a.N, a.K, k, p0, nvalid);
        __syncthreads();
        const float *src = hidden_fwd_chain<LD, NH>(a, lds, F, L);
        last_compare<LD, NH, NS, true>(src, dzl, cl, cinl, cout, wave, h, j, tgt, dzg, dz0, NoSink{});
        __syncthreads();
        for (int l = L; l >= 2; --l) back_layer<LD, NH>(a, lds, dzl, L, l, NoSink{});
        add_d0<LD, NH, NS>(a, lds, F, wave, h, j, S);
        // (img[1] is written again after the barrier that follows the next gather, which a wave reaches after these reads)
    }
    store_gx<LD, NH, NS>(a, rows, b, p0, nvalid, wave, h, j, S);
}

// ---- the host side -------------------------------------------------------------------------------------------------
// the LDS images: 64 points per block where max(L, 2) of them fit, else 32
void lds_plan(const int32_t *layers, int nlayers, int *ld, int *nh, size_t *bytes) {
    *ld = adjoint_stride(layers, nlayers);
    const int L = nlayers - 1, nimg = L >= 2 ? L : 2;
    const size_t half = (size_t)nimg * 32 * *ld * sizeof(float);
    *nh = 2 * half <= kMaxLds ? 2 : 1;
    *bytes = *nh * half;
}

template <int LD, int NH, int NS>
fx3d_status launch(const AdjointArgs &a, size_t lds_bytes, int B, hipStream_t st) {
    const fx3d_status rc = ensure_dynamic_lds(reinterpret_cast<const void *>(&edgeconv_bwd_kernel<LD, NH, NS>), (int)kMaxLds, "edgeconv_bwd_kernel");
    if (rc != FX3D_OK) return rc;
    ProfileScope prof("edgeconv_bwd", st);
    const int T = 32 * NH;
    hipLaunchKernelGGL((edgeconv_bwd_kernel<LD, NH, NS>), dim3((a.N + T - 1) / T, B), dim3(kPtThreads), lds_bytes, st, a);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

}  // namespace

namespace fx3d {
namespace mlp {

// Wt_l of every layer into `wt` (edgeconv_transposed_floats(layers, nlayers) floats), wt_of[l]: where layer l + 1's begins
size_t edgeconv_transposed_floats(const int32_t *layers, int nlayers) {
    size_t nw = 0;
    for (int i = 1; i < nlayers; ++i) nw += (size_t)(i == 1 ? 2 * layers[0] : layers[i - 1]) * layers[i];
    return nw;
}
fx3d_status edgeconv_transpose_weights(const Conv *c, const int32_t *layers, int nlayers, float *wt, const float **wt_of, hipStream_t st) {
    TransposeArgs t{};
    int most = 1;
    for (int l = 0; l + 1 < nlayers; ++l) {
        t.W[l] = c[l].W;
        t.cin[l] = l == 0 ? 2 * layers[0] : layers[l];
        t.cout[l] = layers[l + 1];
        t.wt[l] = wt;
        wt_of[l] = wt;
        wt += (size_t)t.cin[l] * t.cout[l];
        most = t.cin[l] * t.cout[l] > most ? t.cin[l] * t.cout[l] : most;
    }
    hipLaunchKernelGGL(transpose_weights, dim3((most + 255) / 256, nlayers - 1), dim3(256), 0, st, t);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

// ---- the host preamble of both adjoints (edgeconv_adjoint.h) -----------------------------------------------------------------
fx3d_status edgeconv_adjoint_plan(const char *fn, const int32_t *layers, int nlayers, int N, int B, int K, WsBump &ws, AdjointWs *w) {
    fx3d_status rc = check_layers(fn, layers, nlayers);
    if (rc != FX3D_OK) return rc;
    if ((rc = check_edgeconv_sizes(fn, N, B, K)) != FX3D_OK) return rc;
    if ((rc = edgeconv_workspace_bytes(layers[0], N, B, K, &w->fwd_bytes)) != FX3D_OK) return rc;
    w->fwd = ws.put(w->fwd_bytes);
    w->idx = ws.put((size_t)K * N * B * sizeof(int32_t));
    w->out = ws.put((size_t)layers[nlayers - 1] * N * B * sizeof(float));
    w->wt = ws.put(edgeconv_transposed_floats(layers, nlayers) * sizeof(float));
    return FX3D_OK;
}

fx3d_status edgeconv_adjoint_prepare(const char *fn, const char *size_fn, const AdjointWs &w, size_t need, const float *params_dev,
                                     const int32_t *layers, int nlayers, int K, const float *x, int N, int B, const int32_t *idx,
                                     const float *out, const float *gout, float *gx, void *ws, size_t ws_bytes, fx3d_stream_t s,
                                     AdjointArgs *a, const float *stats) {
    FX3D_REQUIRE(ws_bytes >= need, "%s: workspace of %zu bytes, %s says %zu", fn, ws_bytes, size_fn, need);
    FX3D_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "%s: ws must be 256-byte aligned", fn);
    char *wsb = static_cast<char *>(ws);
    edgeconv_layout(params_dev, layers, nlayers, a->c);
    for (int i = 0; i < nlayers; ++i) a->w[i] = layers[i];
    a->nl = nlayers - 1; a->cout = layers[nlayers - 1];
    a->N = N; a->K = K; a->x = x; a->gout = gout; a->gx = gx;
    // the forward's part: the lists and / or out where the caller has none (the search is deterministic: the forward's lists)
    int32_t *ws_idx = reinterpret_cast<int32_t *>(wsb + w.idx);
    float *ws_out = reinterpret_cast<float *>(wsb + w.out);
    fx3d_status r = FX3D_OK;
    if (stats) {  // edge_pass puts the statistics in the BatchNorms' place: the closing pass of the training-mode forward
        const int32_t *used = nullptr;
        if ((r = edgeconv_neighbours(x, layers[0], N, B, K, idx, ws_idx, wsb + w.fwd, s, &used)) != FX3D_OK) return r;
        const EdgePass p = edge_pass(params_dev, stats, layers, nlayers, K, x, N, used, ws_out);
        for (int i = 0; i + 1 < nlayers; ++i) a->c[i].bn = p.a.c[i].bn;
        if (!out && (r = edgeconv_launch(p, B, as_stream(s), "edgeconv_grad_train_forward")) != FX3D_OK) return r;
        idx = used;
    } else if (!out) {
        if ((r = edgeconv_run(params_dev, layers, nlayers, K, x, N, B, idx, ws_out, idx ? nullptr : ws_idx, wsb + w.fwd, s, "edgeconv")) != FX3D_OK) return r;
    } else if (!idx) {
        if ((r = fx3d_knn_ws(x, N, x, N, B, layers[0], K, 1, ws_idx, nullptr, wsb + w.fwd, w.fwd_bytes, s)) != FX3D_OK) return r;
    }
    a->idx = idx ? idx : ws_idx;
    a->out = out ? out : ws_out;
    return edgeconv_transpose_weights(a->c, layers, nlayers, reinterpret_cast<float *>(wsb + w.wt), a->wt, as_stream(s));
}

}  // namespace mlp
}  // namespace fx3d

extern "C" {

fx3d_status fx3d_edgeconv_bwd_workspace_bytes(const int32_t *layers, int32_t nlayers, int32_t K, int32_t N, int32_t B, size_t *bytes) {
    const char *fn = "fx3d_edgeconv_bwd_workspace_bytes";
    FX3D_REQUIRE(bytes != nullptr, "%s: bytes is NULL", fn);
    WsBump ws;
    AdjointWs w;
    const fx3d_status rc = edgeconv_adjoint_plan(fn, layers, nlayers, N, B, K, ws, &w);
    if (rc != FX3D_OK) return rc;
    *bytes = ws.at;
    return FX3D_OK;
}

fx3d_status fx3d_edgeconv_bwd(const float *params_dev, const int32_t *layers, int32_t nlayers, int32_t K, const float *x, int32_t N,
                              int32_t B, const int32_t *idx, const float *out, const float *gout, float *gx, void *ws,
                              size_t ws_bytes, fx3d_stream_t s) {
    const char *fn = "fx3d_edgeconv_bwd";
    FX3D_REQUIRE(params_dev && x && gout && gx && ws, "%s: params_dev, x, gout, gx and ws must not be NULL", fn);
    WsBump bump;
    AdjointWs w;
    AdjointArgs a{};
    fx3d_status r = edgeconv_adjoint_plan(fn, layers, nlayers, N, B, K, bump, &w);
    if (r != FX3D_OK) return r;
    if ((r = edgeconv_adjoint_prepare(fn, "fx3d_edgeconv_bwd_workspace_bytes", w, bump.at, params_dev, layers, nlayers, K, x, N, B,
                                      idx, out, gout, gx, ws, ws_bytes, s, &a)) != FX3D_OK) return r;
    size_t lds_bytes = 0;
    int ld = 0, nh = 0;
    lds_plan(layers, nlayers, &ld, &nh, &lds_bytes);
    hipStream_t st = as_stream(s);
    // the stride 66 holds 64 channels at most: one slab per wave there
    switch (ld) {
        case 66: return launch<66, 2, 1>(a, lds_bytes, B, st);  // (four images are 68 KB: always 64 points)
        case kLd: return nh == 2 ? launch<kLd, 2, 1>(a, lds_bytes, B, st) : launch<kLd, 1, 1>(a, lds_bytes, B, st);
        default: return nh == 2 ? launch<258, 2, 2>(a, lds_bytes, B, st) : launch<258, 1, 2>(a, lds_bytes, B, st);
    }
}

}  // extern "C"
