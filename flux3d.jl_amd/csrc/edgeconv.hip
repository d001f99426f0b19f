// EdgeConv(layers, K) as a layer in its own right (gfx950): (m::EdgeConv)(X) of src/models/dgcnn.jl:11-71 in test mode, Float32,
// forward only, for layer widths chosen at run time.  include/flux3d_hip.h ("EdgeConv inference") states the layer, the
// arithmetic and the parameter layout; this file is how they are computed.  It is the library's one EdgeConv: fx3d_edgeconv_forward
// and both stages of fx3d_dgcnn_forward (dgcnn.hip) go through edgeconv_run below, so EdgeConv([3, 32, 64, 64], K) and
// EdgeConv([64, 128, 256], K) are DGCNN's x1 and x2.  The arithmetic is the contract of mlp_common.h.
//
// Per call: the neighbour search (fx3d_knn_ws on the cloud's own F-dimensional rows, rank 0 dropped) unless the caller gives
// the lists, then edgeconv_kernel<NS, LD>: one block = 64 points of one cloud, 4 waves, looping over the neighbour rank k.
//   LDS: up to three 64-row images of one row stride LD = 66 / 130 / 258 (the smallest that holds the widest layer INPUT;
//     LD mod 64 = 2 is the bank pattern kLd documents; a template parameter, so that an LDS address is a register plus an
//     immediate): `rows` holds the edge rows [x_n, x_idx(k,n) - x_n], img0 and img1 take the hidden layers in turn
//     (rows -> img0 -> img1 -> img0).  L = 1 needs `rows` alone, L = 2 rows and img0.  Three images of stride 258 (198 KB)
//     do not fit the CU's 160 KB (two are 132 KB, kMaxLds): then img1 IS `rows`, and the x_n half, otherwise gathered once before the
//     loop, is gathered again with every k (EdgeConvArgs::shared_rows).
//   Per k: gather the second half of the rows; every hidden layer from image to image (conv_rt: the MFMA over the first
//     4 floor(Cin / 4) input channels, v_fma_f32 on the accumulator for the rest, mfma_slab_rt); the LAST layer is never stored
//     but folded into a running Julia max per (point, channel) in registers (fold_slab): a lane owns one channel and 16 points per
//     32-point half, a wave the slabs wave, wave + 4 of 32 channels.  NS = 1 up to 128 output channels, NS = 2 (64 VGPRs
//     of maxima) up to 256.  A layer of up to 64 channels has two slabs at most: there a wave takes one HALF of one slab, so
//     that no wave idles (split_halves).
//   An output width that is no multiple of 32 leaves the last slab partial: its lanes beyond the width read the parameters of
//     the last channel (inside the buffer), run the wave's MFMAs with them and write nothing.
//   Rows beyond the cloud's last point are zeros: computed, never written.  After the last k, plain stores (fold_store).
// The kernel's arguments, a hidden layer (conv_rt), the loop over k with its last layer left to the caller (edge_trunk), the LDS
// plan and the workspace are in edgeconv_net.h, which the training-mode forward (edgeconv_train.hip) shares: its statistics
// passes are that loop stopped at a BatchNorm.
#include "edgeconv_net.h"

using namespace fx3d;
using namespace fx3d::mlp;

namespace {

// the last layer for the current k, folded into the wave's running maxima (split_halves: into rm0[0] alone)
template <int NS, int LD>
__device__ __forceinline__ void conv_rt_fold(const float *in, int cin, int cout, const Conv &c, f32x16 (&rm0)[NS],
                                             f32x16 (&rm1)[NS]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, j = lane & 31;
    if (NS == 1 && split_halves(cout)) {
        if ((wave >> 1) * 32 >= cout) return;
        const int oc = min((wave >> 1) * 32 + j, cout - 1);  // (a lane beyond a partial slab folds the last channel; never stored)
        f32x16 acc[1] = {f32x16{0}};
        mfma_slab_rt<LD, 1>(in + (wave & 1) * 32 * LD, c.W + (size_t)cin * oc, cin, h, j, acc);
        fold_half(acc[0], c, oc, rm0[0]);
        return;
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int sl = wave + s * (kPtThreads / 64);
        if (sl * 32 >= cout) break;  // wave-uniform
        const int oc = min(sl * 32 + j, cout - 1);
        f32x16 acc[2] = {f32x16{0}, f32x16{0}};
        mfma_slab_rt<LD, 2>(in, c.W + (size_t)cin * oc, cin, h, j, acc);
        fold_slab(acc[0], acc[1], c, oc, rm0[s], rm1[s]);
    }
}

// fold_store for split_halves: the wave's half of its slab
__device__ __forceinline__ void fold_store_half(float *ob, int cout, int nvalid, const f32x16 &rm) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, j = lane & 31;
    const int o = (wave >> 1) * 32 + j;
    if (o >= cout) return;  // a wave without a slab, the lanes beyond a partial slab
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int p = (wave & 1) * 32 + mfma_row(r, h);
        if (p < nvalid) ob[(size_t)p * cout + o] = rm[r];
    }
}

template <int NS, int LD>
__global__ __launch_bounds__(kPtThreads) void edgeconv_kernel(const EdgeConvArgs a) {
    extern __shared__ float lds[];
    const int tile = blockIdx.x, b = blockIdx.y;
    const int p0 = tile * kTile;
    const int nvalid = min(kTile, a.N - p0);
    const int cout = a.cout;
    f32x16 rm0[NS], rm1[NS];
    fold_init<NS>(rm0, rm1);
    // the loop over k (edge_trunk, edgeconv_net.h), its last layer folded into the running maxima
    edge_trunk<LD>(a, lds, b, p0, nvalid,
                   [&](const float *src, int cin, int co, const Conv &c) { conv_rt_fold<NS, LD>(src, cin, co, c, rm0, rm1); });
    float *ob = a.out + ((size_t)b * a.N + p0) * cout;
    if (NS == 1 && split_halves(cout)) fold_store_half(ob, cout, nvalid, rm0[0]);
    else fold_store<NS>(ob, cout, nvalid, rm0, rm1);
}

// ---- the host side (the LDS plan, the workspace and a pass's arguments: edgeconv_net.h) ------------------------------------------
template <int NS, int LD>
fx3d_status launch(const EdgeConvArgs &a, size_t lds_bytes, int B, hipStream_t st, const char *label) {
    const fx3d_status rc = ensure_dynamic_lds(reinterpret_cast<const void *>(&edgeconv_kernel<NS, LD>), (int)kMaxLds, "edgeconv_kernel");
    if (rc != FX3D_OK) return rc;
    ProfileScope prof(label, st);
    hipLaunchKernelGGL((edgeconv_kernel<NS, LD>), dim3((a.N + kTile - 1) / kTile, B), dim3(kPtThreads), lds_bytes, st, a);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

}  // namespace

// ---- the entry the model units share (mlp_common.h) -----------------------------------------------------------------------
namespace fx3d {
namespace mlp {

// the flat parameter buffer: per block conv W (Cin, Cout), b, then BatchNorm gamma, beta, mu, var
long long edgeconv_layout(const float *params, const int32_t *layers, int nlayers, Conv *c) {
    Cursor cur{params, 0};
    for (int i = 1; i < nlayers; ++i) {
        Conv v = cur.conv(i == 1 ? 2 * layers[0] : layers[i - 1], layers[i]);
        v.bn = cur.bn(layers[i]);
        if (c) c[i - 1] = v;
    }
    return cur.at;
}

fx3d_status edgeconv_workspace_bytes(int F, int N, int B, int K, size_t *bytes) {
    EdgeWsPlan w;
    const fx3d_status rc = edge_ws_plan(F, N, B, K, &w);
    if (rc != FX3D_OK) return rc;
    *bytes = w.total;
    return FX3D_OK;
}

fx3d_status edgeconv_neighbours(const float *x, int F, int N, int B, int K, const int32_t *idx_in, int32_t *idx_out, void *ws,
                                fx3d_stream_t s, const int32_t **idx) {
    *idx = idx_in;
    if (idx_in) return FX3D_OK;
    EdgeWsPlan w;
    const fx3d_status r = edge_ws_plan(F, N, B, K, &w);
    if (r != FX3D_OK) return r;
    char *wsb = static_cast<char *>(ws);
    int32_t *found = idx_out ? idx_out : reinterpret_cast<int32_t *>(wsb + w.idx);
    *idx = found;
    return fx3d_knn_ws(x, N, x, N, B, F, K, 1, found, nullptr, w.knn_bytes ? wsb + w.knn : nullptr, w.knn_bytes, s);
}

fx3d_status edgeconv_launch(const EdgePass &p, int B, hipStream_t st, const char *label) {
    const EdgeConvArgs &a = p.a;
    const bool wide = a.cout > 128;  // two slabs of running maxima per wave
    switch (p.ld) {
        case 66: return wide ? launch<2, 66>(a, p.lds_bytes, B, st, label) : launch<1, 66>(a, p.lds_bytes, B, st, label);
        case kLd: return wide ? launch<2, kLd>(a, p.lds_bytes, B, st, label) : launch<1, kLd>(a, p.lds_bytes, B, st, label);
        default: return wide ? launch<2, 258>(a, p.lds_bytes, B, st, label) : launch<1, 258>(a, p.lds_bytes, B, st, label);
    }
}

fx3d_status edgeconv_run(const float *params_dev, const int32_t *layers, int nlayers, int K, const float *x, int N, int B,
                         const int32_t *idx_in, float *out, int32_t *idx_out, void *ws, fx3d_stream_t s, const char *label) {
    const int32_t *idx = nullptr;
    const fx3d_status r = edgeconv_neighbours(x, layers[0], N, B, K, idx_in, idx_out, ws, s, &idx);
    if (r != FX3D_OK) return r;
    return edgeconv_launch(edge_pass(params_dev, nullptr, layers, nlayers, K, x, N, idx, out), B, as_stream(s), label);
}

}  // namespace mlp
}  // namespace fx3d

extern "C" {

fx3d_status fx3d_edgeconv_param_count(const int32_t *layers, int32_t nlayers, int64_t *count) {
    const char *fn = "fx3d_edgeconv_param_count";
    FX3D_REQUIRE(count != nullptr, "%s: count is NULL", fn);
    const fx3d_status rc = check_layers(fn, layers, nlayers);
    if (rc != FX3D_OK) return rc;
    *count = edgeconv_layout(nullptr, layers, nlayers, nullptr);
    return FX3D_OK;
}

fx3d_status fx3d_edgeconv_workspace_bytes(const int32_t *layers, int32_t nlayers, int32_t K, int32_t N, int32_t B, size_t *bytes) {
    const char *fn = "fx3d_edgeconv_workspace_bytes";
    FX3D_REQUIRE(bytes != nullptr, "%s: bytes is NULL", fn);
    fx3d_status rc = check_layers(fn, layers, nlayers);
    if (rc != FX3D_OK) return rc;
    if ((rc = check_edgeconv_sizes(fn, N, B, K)) != FX3D_OK) return rc;
    return edgeconv_workspace_bytes(layers[0], N, B, K, bytes);
}

fx3d_status fx3d_edgeconv_forward(const float *params_dev, const int32_t *layers, int32_t nlayers, int32_t K, const float *x,
                                  int32_t N, int32_t B, const int32_t *idx_in, float *out, int32_t *idx_out, void *ws,
                                  size_t ws_bytes, fx3d_stream_t s) {
    const char *fn = "fx3d_edgeconv_forward";
    FX3D_REQUIRE(params_dev && x && out && ws, "%s: params_dev, x, out and ws must not be NULL", fn);
    fx3d_status r = check_layers(fn, layers, nlayers);
    if (r != FX3D_OK) return r;
    if ((r = check_edgeconv_sizes(fn, N, B, K)) != FX3D_OK) return r;
    size_t need = 0;
    if ((r = edgeconv_workspace_bytes(layers[0], N, B, K, &need)) != FX3D_OK) return r;
    FX3D_REQUIRE(ws_bytes >= need, "%s: workspace of %zu bytes, fx3d_edgeconv_workspace_bytes says %zu", fn, ws_bytes, need);
    FX3D_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "%s: ws must be 256-byte aligned", fn);
    return edgeconv_run(params_dev, layers, nlayers, K, x, N, B, idx_in, out, idx_out, ws, s, "edgeconv");
}

}  // extern "C"
