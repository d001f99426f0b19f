// EdgeConv(layers, K): the gradients with respect to the parameters (conv W and b, BatchNorm gamma and beta; test-mode
// BatchNorm) and, when asked, with respect to the input, from one fused kernel (gfx950).  include/flux3d_hip.h ("EdgeConv
// parameter adjoint") states the definition and the order of every sum; tests/edgeconv_pgrad_ref.py restates it on the host.
//
// The chain is the input adjoint's (edgeconv_bwd.hip), step by step the functions of edgeconv_adjoint.h that it calls: per
// neighbour rank k the forward tile is recomputed (gather_rows, hidden_fwd_chain), the k that took the maximum found
// (last_compare), and the layers walked back (back_layer, add_d0; store_gx per tile).  Where that kernel gives the steps empty
// sinks, this one contracts a layer's upstream gradient d_l with the layer's input, which is still in its LDS image (take):
//   H_l[c,o] += sum over the tile's rows of a_{l-1}[row][c] d_l[row][o],   h_l[o] += sum of d_l[row][o].
// edgeconv_pgrad_kernel<LD, NS, NT>: one block = one chunk of kGradChunk = 128 consecutive points of one cloud = up to four
//   32-point tiles, one after the other, 4 waves, looping over k inside a tile.  gridDim = (chunks, B, passes).
//   The contraction: the lane that produces d_l[row][o] for its channel o holds its 16 rows mfma_row(r, h) in registers (the
//     compare step for layer L, hidden_bwd's accumulators for the others).  They are the B operand of v_mfma_f32_32x32x2f32 as
//     they stand: MFMA r contracts the two rows mfma_row(r, 0) (lanes 0-31) and mfma_row(r, 1) (lanes 32-63), in this order.
//     The A operand is a_{l-1}[mfma_row(r, h)][c0 + lane % 32] from LDS: consecutive words per half-wave.  The result tile is
//     H_l[c0 + mfma_row(r', h)][o0 + lane % 32]: 16 registers per lane per (32 input channels) x (32 output channels).
//     Rows beyond the cloud's last point have d = +0 in the registers: every product is a zero and the chain, which began at
//     +0 and therefore never holds -0, does not change.  Channel tails: the index is clamped, the tile computed, not written.
//   The accumulators: wave w owns the output slabs w, w + 4, ... of every layer (the forward's ownership), times all of the
//     layer's ceil(cin / 32) input tiles -- its tile list, layer by layer.  NT of them live in registers across the tiles and k
//     of a chunk; pass z (blockIdx.z) of a block takes tiles z NT .. z NT + NT - 1 of every wave's list and recomputes the chain.
//     An element of H has one owner in one pass: the passes change no bit.  A later pass holds later layers only and ends its
//     walk back at the lowest of them (PgradArgs::lmin); pass 0 walks all the way and owns gx.
//     After the chunk: one plain store per element into the chunk's partial slab (the parameter buffer's layout: H_l in W_l's
//     place, h_l in b_l's).  No atomics.
//   h_l[o]: two chains per chunk, one per half-wave (rows mfma_row(r, 0) and mfma_row(r, 1)), added once at the flush; pass 0.
//   LDS: images of 32 rows, stride LD as the adjoint.  L = 1: rows, dz_1.  L = 2: rows, a_1 / dz_1, dz_2 (d_1 is contracted with
//     the edge rows, which must outlive dz_2).  L >= 3: L images, dz_L in `rows`' place as in the adjoint, and the edge rows
//     gathered again for the same k once hidden_bwd(L) has consumed dz_L.  Four images of stride 258 are 132 KB.
//   gx (pass 0, when asked): the adjoint's sums S and subtraction, per tile.  Unlike the input adjoint this kernel keeps gout as
//     it is (gv) and scales at the compare (last_compare with SCALED = false): d_L is what it contracts.
// Then pgrad_reduce (the chunk partials of every H and h element as one chain, b ascending, chunk ascending) and pgrad_finish
// (the four families from H and h).
// The kernel, take, its plan and its launch are in edgeconv_pgrad_net.h: the training-mode adjoint (edgeconv_grad_train.hip) closes with
// the same kernel on PgradTrainArgs and with pgrad_reduce (launch_pgrad_reduce below).
#include "edgeconv_pgrad_net.h"

using namespace fx3d;
using namespace fx3d::mlp;

namespace {

// sums[e] = the chain from +0 over the chunk partials, b ascending, chunk ascending, for the elements of every H_l and h_l
__global__ __launch_bounds__(256) void pgrad_reduce(const FinishArgs f) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    int l, at;
    if (e >= f.psize || !locate(f, e, &l, &at)) return;
    const int cin = l == 0 ? f.cin[0] : l == 1 ? f.cin[1] : l == 2 ? f.cin[2] : f.cin[3];
    const int cout = l == 0 ? f.cout[0] : l == 1 ? f.cout[1] : l == 2 ? f.cout[2] : f.cout[3];
    if (at >= (cin + 1) * cout) return;  // gamma, beta, mu, var: no sums
    float acc = 0.0f;
    for (int p = 0; p < f.nparts; ++p) acc = acc + f.part[(size_t)p * f.psize + e];
    f.sums[e] = acc;
}

// the four families from H and h (flux3d_hip.h); mu and var: +0
__global__ __launch_bounds__(256) void pgrad_finish(const FinishArgs f) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    int l, at;
    if (e >= f.psize || !locate(f, e, &l, &at)) return;
    const Conv c = l == 0 ? f.c[0] : l == 1 ? f.c[1] : l == 2 ? f.c[2] : f.c[3];
    const int cin = l == 0 ? f.cin[0] : l == 1 ? f.cin[1] : l == 2 ? f.cin[2] : f.cin[3];
    const int cout = l == 0 ? f.cout[0] : l == 1 ? f.cout[1] : l == 2 ? f.cout[2] : f.cout[3];
    const int woff = l == 0 ? f.woff[0] : l == 1 ? f.woff[1] : l == 2 ? f.woff[2] : f.woff[3];
    const float *Hs = f.sums + woff, *hs = Hs + cin * cout;
    const int nw = cin * cout;
    float v = 0.0f;
    if (at < nw) {  // dW[c,o] = (H[c,o] gamma[o]) / sd[o]
        const int o = at / cin;
        v = (Hs[at] * c.bn.g[o]) / sqrtf(c.bn.v[o] + kBnEps);
    } else {
        const int fam = (at - nw) / cout, o = at - nw - fam * cout;
        const float sd = sqrtf(c.bn.v[o] + kBnEps);
        if (fam == 0) {  // db
            v = (hs[o] * c.bn.g[o]) / sd;
        } else if (fam == 1) {  // dgamma
            float acc = 0.0f;
            for (int i = 0; i < cin; ++i) acc = fmaf(c.W[i + cin * o], Hs[i + cin * o], acc);
            v = (acc + (c.b[o] - c.bn.m[o]) * hs[o]) / sd;
        } else if (fam == 2) {  // dbeta
            v = hs[o];
        }
    }
    f.g[e] = v;
}

}  // namespace

namespace fx3d {
namespace mlp {

fx3d_status launch_pgrad_reduce(const FinishArgs &f, hipStream_t st) {
    hipLaunchKernelGGL(pgrad_reduce, dim3((f.psize + 255) / 256), dim3(256), 0, st, f);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

}  // namespace mlp
}  // namespace fx3d

extern "C" {

fx3d_status fx3d_edgeconv_grad_workspace_bytes(const int32_t *layers, int32_t nlayers, int32_t K, int32_t N, int32_t B, size_t *bytes) {
    const char *fn = "fx3d_edgeconv_grad_workspace_bytes";
    FX3D_REQUIRE(bytes != nullptr, "%s: bytes is NULL", fn);
    WsPlan w;
    const fx3d_status rc = ws_plan(fn, layers, nlayers, N, B, K, &w);
    if (rc != FX3D_OK) return rc;
    *bytes = w.total;
    return FX3D_OK;
}

fx3d_status fx3d_edgeconv_grad(const float *params_dev, const int32_t *layers, int32_t nlayers, int32_t K, const float *x, int32_t N,
                               int32_t B, const int32_t *idx, const float *out, const float *gout, float *gparams, float *gx,
                               void *ws, size_t ws_bytes, fx3d_stream_t s) {
    const char *fn = "fx3d_edgeconv_grad";
    FX3D_REQUIRE(params_dev && x && gout && gparams && ws, "%s: params_dev, x, gout, gparams and ws must not be NULL", fn);
    WsPlan w;
    PgradArgs a{};
    FinishArgs f{};
    fx3d_status r = ws_plan(fn, layers, nlayers, N, B, K, &w);
    if (r != FX3D_OK) return r;
    if ((r = edgeconv_adjoint_prepare(fn, "fx3d_edgeconv_grad_workspace_bytes", w.adj, w.total, params_dev, layers, nlayers, K, x, N, B,
                                      idx, out, gout, gx, ws, ws_bytes, s, &a)) != FX3D_OK) return r;
    hipStream_t st = as_stream(s);
    const Plan p = plan(layers, nlayers);
    pgrad_fill(params_dev, layers, nlayers, w, p, B, ws, &a, &f);
    const char *label = "edgeconv_pgrad";
    switch (p.ld) {
        case 66: r = launch_pgrad<66, 1, kTilesNarrow>(a, p, w.chunks, B, st, label); break;
        case kLd: r = launch_pgrad<kLd, 1, kTilesNarrow>(a, p, w.chunks, B, st, label); break;
        default: r = launch_pgrad<258, 2, kTilesWide>(a, p, w.chunks, B, st, label); break;
    }
    if (r != FX3D_OK) return r;
    f.g = gparams;
    ProfileScope prof("edgeconv_pgrad_finish", st);
    if ((r = launch_pgrad_reduce(f, st)) != FX3D_OK) return r;
    hipLaunchKernelGGL(pgrad_finish, dim3((f.psize + 255) / 256), dim3(256), 0, st, f);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

}  // extern "C"
