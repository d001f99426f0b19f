// DGCNN's adjoint (gfx950): the gradients of sum(glogits . logits) with respect to every parameter of the network and to the
// input points, test mode, Float32.  include/flux3d_hip.h ("DGCNN adjoint") states the definition and the order of every sum;
// tests/dgcnn_grad_ref.py restates it on the host.  The two EdgeConv stages are fx3d_edgeconv_grad itself (edgeconv_pgrad.hip),
// called on the ec2 and then the ec1 slice of the parameter buffer; this file is the tail: conv_3, the maximum over the
// points, fc_4, fc_5, fc_6.
//
// The maximum over the N points picks ONE point per (channel, cloud), so conv_3's adjoint is a gather: 1024 rows of W3 per cloud
// for gx2 and 1024 rows of x2 per cloud for H3, not the dense (256 x 1024 x N) contractions.  Per call, after the forward where
// the caller gives no intermediates:
//   dgcnn_argmax_kernel (dgcnn_net.h's conv3_winners, shared with the training-mode adjoint): the forward's conv_3 again, block for
//     block (64 points, the x2 tile in one LDS image of stride 258, mfma_slab<256> and epilogue<kBnRelu>: the forward's bits),
//     compared with pooled where that is positive; per (tile, channel) the smallest matching point, a lane minimum over its 32 rows
//     and one shuffle across the half-waves (the forward's fold).
//   dgcnn_head_bwd_kernel: one block per cloud.  Thread c folds the tile minima of channel c into n*(c); a4 and a5 are computed
//     again as the forward's head computes them (dense_chain); then g5, d5, g4, d4 and gp, one thread per element, each one chain
//     over the layer's outputs (transposed_chain: a thread's weights are one contiguous row of the (out, in) array).  a4, a5, d5,
//     d4, d3, dz3 and n* go to the workspace.
//   dgcnn_gx2_kernel: one block = 64 points of one cloud, a wave owns a point's 256 outputs (4 per lane).  The cloud's n* and dz3
//     are in LDS; the wave finds its point's channels 64 at a time with a ballot and walks them in ascending order.  A point
//     that wins nothing gets +0.  No atomics: a point has one owner.
//   dgcnn_conv3_pgrad_kernel: one block per output channel c, thread i owns H3[i, c]: the chain over the clouds that have a
//     winner of x2[i, n*(c, b), b] d3[c, b]; then the four families of the channel.
//   dense_sums_kernel (pointnet_grad.hip's, through launch_dense_sums; fc_4, fc_5, fc_6): one thread per element of H and h, the
//     chain over the clouds.  fc_6's go to gparams as they are.  dense_finish_kernel (fc_4, fc_5): the four families from H and h,
//     one thread per element of the layer's block.
//   fx3d_edgeconv_grad on ec2 (gout = gx2 -> gx1), then on ec1 (gout = gx1 -> gx).
#include "dgcnn_net.h"

using namespace fx3d;
using namespace fx3d::mlp;
using pointnet::grad_block;
using pointnet::GradBlock;
using pointnet::kNoPoint;
using pointnet::mut;

namespace {

// the winners: dgcnn_net.h's conv3_winners
__global__ __launch_bounds__(kPtThreads) void dgcnn_argmax_kernel(const float *__restrict__ x2, const Conv c,
                                                                  const float *__restrict__ pooled, int32_t *__restrict__ tfirst,
                                                                  int N, int ntiles) {
    extern __shared__ float lds[];
    conv3_winners<false>(lds, x2, c, pooled, tfirst, nullptr, N, ntiles);
}

struct HeadBwdArgs {
    const int32_t *tfirst;  // (1024, ntiles, B)
    int ntiles, nc;
    const float *pooled;    // (1024, B)
    const float *glogits;   // (nc, B) = d6
    Conv c3;
    Dense d4, d5, d6;
    Bn bn4, bn5;
    int32_t *nstar;         // (1024, B): the winning point, -1 where there is none
    float *a4, *a5, *g5, *g4, *d3, *dz3;  // a4 (512, B), a5 (256, B), d5 (256, B), d4 (512, B), d3 and dz3 (1024, B)
};

__global__ __launch_bounds__(kHeadThreads) void dgcnn_head_bwd_kernel(const HeadBwdArgs a) {
    __shared__ float v0[kFeat], v1[512], v2[256], z1[512], z2[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    // n*(c): the smallest point over the tiles
    int first = kNoPoint;
    {
        const int32_t *t = a.tfirst + (size_t)b * a.ntiles * kFeat + tid;
        for (int k = 0; k < a.ntiles; ++k) first = min(first, t[(size_t)k * kFeat]);
    }
    const bool won = first != kNoPoint;
    a.nstar[(size_t)b * kFeat + tid] = won ? first : -1;
    v0[tid] = a.pooled[(size_t)b * kFeat + tid];
    __syncthreads();
    // the forward's head again: a4, a5
    if (tid < 512) {
        const float v = dense_chain(v0, kFeat, a.d4.W, 512, tid) + a.d4.b[tid];
        v1[tid] = relu(batchnorm(v, a.bn4.g[tid], a.bn4.b[tid], a.bn4.m[tid], sqrtf(a.bn4.v[tid] + kBnEps)));
        a.a4[(size_t)b * 512 + tid] = v1[tid];
    }
    __syncthreads();
    if (tid < 256) {
        const float v = dense_chain(v1, 512, a.d5.W, 256, tid) + a.d5.b[tid];
        v2[tid] = relu(batchnorm(v, a.bn5.g[tid], a.bn5.b[tid], a.bn5.m[tid], sqrtf(a.bn5.v[tid] + kBnEps)));
        a.a5[(size_t)b * 256 + tid] = v2[tid];
        // g5 = the chain over the classes, d5, dz5
        const float *d6 = a.glogits + (size_t)b * a.nc, *w = a.d6.W + (size_t)a.nc * tid;
        float acc = 0.0f;
        for (int o = 0; o < a.nc; ++o) acc = fmaf(d6[o], w[o], acc);
        const float d = v2[tid] > 0.0f ? acc : 0.0f;
        a.g5[(size_t)b * 256 + tid] = d;
        z2[tid] = (d * a.bn5.g[tid]) / sqrtf(a.bn5.v[tid] + kBnEps);
    }
    __syncthreads();
    if (tid < 512) {
        const float g4 = transposed_chain(z2, 256, a.d5.W, tid);
        const float d = v1[tid] > 0.0f ? g4 : 0.0f;
        a.g4[(size_t)b * 512 + tid] = d;
        z1[tid] = (d * a.bn4.g[tid]) / sqrtf(a.bn4.v[tid] + kBnEps);
    }
    __syncthreads();
    const float gp = transposed_chain(z1, 512, a.d4.W, tid);
    const float d3 = won ? gp : 0.0f;
    a.d3[(size_t)b * kFeat + tid] = d3;
    a.dz3[(size_t)b * kFeat + tid] = (d3 * a.c3.bn.g[tid]) / sqrtf(a.c3.bn.v[tid] + kBnEps);
}

__global__ __launch_bounds__(kPtThreads) void dgcnn_gx2_kernel(const int32_t *__restrict__ nstar, const float *__restrict__ dz3,
                                                               const float *__restrict__ W3, float *__restrict__ gx2, int N) {
    __shared__ int32_t ns[kFeat];
    __shared__ float dz[kFeat];
    const int b = blockIdx.y, p0 = blockIdx.x * kTile;
    for (int c = threadIdx.x; c < kFeat; c += kPtThreads) {
        ns[c] = nstar[(size_t)b * kFeat + c];
        dz[c] = dz3[(size_t)b * kFeat + c];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int p = wave; p < kTile; p += kPtThreads / 64) {
        const int n = p0 + p;
        if (n >= N) break;  // wave-uniform
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int cc = 0; cc < kFeat; cc += 64) {
            unsigned long long m = __ballot(ns[cc + lane] == n);
            while (m) {  // the point's channels among these 64, ascending
                const int c = cc + __ffsll((long long)m) - 1;
                m &= m - 1;
                const float d = dz[c];
                const float *w = W3 + (size_t)256 * c + lane;
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] = fmaf(d, w[64 * q], acc[q]);
            }
        }
        float *g = gx2 + ((size_t)b * N + n) * 256 + lane;
#pragma unroll
        for (int q = 0; q < 4; ++q) g[64 * q] = acc[q];
    }
}

__global__ __launch_bounds__(256) void dgcnn_conv3_pgrad_kernel(const float *__restrict__ x2, const int32_t *__restrict__ nstar,
                                                                const float *__restrict__ d3, const Conv c3, const GradBlock g,
                                                                int N, int B) {
    __shared__ float Hs[256];
    const int c = blockIdx.x, i = threadIdx.x;
    float H = 0.0f, h = 0.0f;
    for (int b = 0; b < B; ++b) {
        const int n = nstar[(size_t)b * kFeat + c];
        if (n < 0) continue;  // block-uniform: the clouds that have a winner
        const float d = d3[(size_t)b * kFeat + c];
        H = fmaf(x2[((size_t)b * N + n) * 256 + i], d, H);
        h = h + d;
    }
    const float gamma = c3.bn.g[c], sd = sqrtf(c3.bn.v[c] + kBnEps);
    g.W[i + (size_t)256 * c] = (H * gamma) / sd;
    Hs[i] = H;
    __syncthreads();
    if (i == 0) {
        float acc = 0.0f;
        const float *w = c3.W + (size_t)256 * c;
        for (int k = 0; k < 256; ++k) acc = fmaf(w[k], Hs[k], acc);
        g.b[c] = (h * gamma) / sd;
        g.g[c] = (acc + (c3.b[c] - c3.bn.m[c]) * h) / sd;
        g.be[c] = h;
        g.m[c] = 0.0f;
        g.v[c] = 0.0f;
    }
}

// the four families of a dense layer with BatchNorm from H and h (flux3d_hip.h); mu and var: +0
struct DenseFinish { const float *H, *h; Dense d; Bn bn; int nin, nout; GradBlock g; };
__global__ __launch_bounds__(256) void dense_finish_kernel(const DenseFinish f) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x, nw = f.nin * f.nout;
    if (e >= nw + 5 * f.nout) return;
    if (e < nw) {  // dW[o,i] = (H[o,i] gamma[o]) / sd[o]
        const int o = e % f.nout;
        f.g.W[e] = (f.H[e] * f.bn.g[o]) / sqrtf(f.bn.v[o] + kBnEps);
        return;
    }
    const int fam = (e - nw) / f.nout, o = e - nw - fam * f.nout;
    const float sd = sqrtf(f.bn.v[o] + kBnEps), h = f.h[o];
    if (fam == 0) {
        f.g.b[o] = (h * f.bn.g[o]) / sd;
    } else if (fam == 1) {
        float acc = 0.0f;
#pragma unroll 16
        for (int i = 0; i < f.nin; ++i) acc = fmaf(f.d.W[o + (size_t)f.nout * i], f.H[o + (size_t)f.nout * i], acc);  // (the loads of 16 steps in flight)
        f.g.g[o] = (acc + (f.d.b[o] - f.bn.m[o]) * h) / sd;
    } else if (fam == 2) {
        f.g.be[o] = h;
    } else if (fam == 3) {
        f.g.m[o] = 0.0f;
    } else {
        f.g.v[o] = 0.0f;
    }
}

// the gradient's block of a dense layer with its BatchNorm
GradBlock dense_block(const Dense &d, const Bn &bn) {
    GradBlock g = grad_block(bn);
    g.W = mut(d.W); g.b = mut(d.b);
    return g;
}

// The workspace: the forward's intermediates and probabilities (used where the caller gives none) | the per-tile first
// matches | n* | a4, a5, d5, d4, d3, dz3 | H and h of fc_4 and fc_5 | gx2, gx1 (used where the caller gives none) | one scratch
// region, the largest of the forward's workspace and the two stages' fx3d_edgeconv_grad workspaces, which use it in turn
struct WsPlan {
    size_t idx1, x1, idx2, x2, pooled, probs, tfirst, nstar, a4, a5, d5, d4, d3, dz3, sums, gx2, gx1, scratch, total;
    size_t fwd_bytes, ec1_bytes, ec2_bytes;
    int ntiles;
};
constexpr size_t kSums = (size_t)kFeat * 512 + 512 + (size_t)512 * 256 + 256;  // H4 | h4 | H5 | h5

fx3d_status ws_plan(int N, int B, int K, int nc, WsPlan *w) {
    w->ntiles = (N + kTile - 1) / kTile;
    const size_t nb = (size_t)N * B;
    WsBump ws;
    w->idx1 = ws.put(nb * K * sizeof(int32_t));
    w->x1 = ws.put(nb * 64 * sizeof(float));
    w->idx2 = ws.put(nb * K * sizeof(int32_t));
    w->x2 = ws.put(nb * 256 * sizeof(float));
    w->pooled = ws.put((size_t)kFeat * B * sizeof(float));
    w->probs = ws.put((size_t)nc * B * sizeof(float));
    w->tfirst = ws.put((size_t)kFeat * w->ntiles * B * sizeof(int32_t));
    w->nstar = ws.put((size_t)kFeat * B * sizeof(int32_t));
    w->a4 = ws.put((size_t)512 * B * sizeof(float));
    w->a5 = ws.put((size_t)256 * B * sizeof(float));
    w->d5 = ws.put((size_t)256 * B * sizeof(float));
    w->d4 = ws.put((size_t)512 * B * sizeof(float));
    w->d3 = ws.put((size_t)kFeat * B * sizeof(float));
    w->dz3 = ws.put((size_t)kFeat * B * sizeof(float));
    w->sums = ws.put(kSums * sizeof(float));
    w->gx2 = ws.put(nb * 256 * sizeof(float));
    w->gx1 = ws.put(nb * 64 * sizeof(float));
    fx3d_status rc;
    if ((rc = fx3d_dgcnn_workspace_bytes(N, B, K, nc, &w->fwd_bytes)) != FX3D_OK) return rc;
    if ((rc = fx3d_edgeconv_grad_workspace_bytes(kEc1, 4, K, N, B, &w->ec1_bytes)) != FX3D_OK) return rc;
    if ((rc = fx3d_edgeconv_grad_workspace_bytes(kEc2, 3, K, N, B, &w->ec2_bytes)) != FX3D_OK) return rc;
    const size_t ec = w->ec1_bytes > w->ec2_bytes ? w->ec1_bytes : w->ec2_bytes;
    w->scratch = ws.put(ec > w->fwd_bytes ? ec : w->fwd_bytes);
    w->total = ws.at;
    return FX3D_OK;
}

}  // namespace

extern "C" {

fx3d_status fx3d_dgcnn_grad_workspace_bytes(int32_t N, int32_t B, int32_t K, int32_t num_classes, size_t *bytes) {
    FX3D_REQUIRE(bytes != nullptr, "fx3d_dgcnn_grad_workspace_bytes: bytes is NULL");
    fx3d_status rc = dgcnn_check_sizes("fx3d_dgcnn_grad_workspace_bytes", N, B, K, num_classes);
    if (rc != FX3D_OK) return rc;
    WsPlan w;
    if ((rc = ws_plan(N, B, K, num_classes, &w)) != FX3D_OK) return rc;
    *bytes = w.total;
    return FX3D_OK;
}

fx3d_status fx3d_dgcnn_grad(const float *params_dev, int32_t num_classes, int32_t K, const float *x, int32_t N, int32_t B,
                            const int32_t *idx1, const float *x1, const int32_t *idx2, const float *x2, const float *pooled,
                            const float *glogits, float *gparams, float *gx, float *gx2, float *gx1, void *ws, size_t ws_bytes,
                            fx3d_stream_t s) {
    const char *fn = "fx3d_dgcnn_grad";
    FX3D_REQUIRE(params_dev && x && glogits && gparams && ws, "%s: params_dev, x, glogits, gparams and ws must not be NULL", fn);
    const int given = (idx1 != nullptr) + (x1 != nullptr) + (idx2 != nullptr) + (x2 != nullptr) + (pooled != nullptr);
    FX3D_REQUIRE(given == 0 || given == 5, "%s: idx1, x1, idx2, x2 and pooled must be given all five or none, got %d of them", fn, given);
    fx3d_status r = dgcnn_check_sizes(fn, N, B, K, num_classes);
    if (r != FX3D_OK) return r;
    WsPlan w;
    if ((r = ws_plan(N, B, K, num_classes, &w)) != FX3D_OK) return r;
    FX3D_REQUIRE(ws_bytes >= w.total, "%s: workspace of %zu bytes, fx3d_dgcnn_grad_workspace_bytes says %zu", fn, ws_bytes, w.total);
    FX3D_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "%s: ws must be 256-byte aligned", fn);
    const Net n = dgcnn_layout(params_dev, num_classes), gn = dgcnn_layout(gparams, num_classes);
    hipStream_t st = as_stream(s);
    char *wsb = static_cast<char *>(ws);
    const pointnet::WsView v{wsb};

    if (given == 0) {  // the forward, into the workspace
        if ((r = fx3d_dgcnn_forward(params_dev, num_classes, K, x, N, B, v.f32(w.probs), nullptr, v.i32(w.idx1), v.f32(w.x1), v.i32(w.idx2),
                                    v.f32(w.x2), v.f32(w.pooled), wsb + w.scratch, w.fwd_bytes, s)) != FX3D_OK) return r;
        idx1 = v.i32(w.idx1); x1 = v.f32(w.x1); idx2 = v.i32(w.idx2); x2 = v.f32(w.x2); pooled = v.f32(w.pooled);
    }
    float *g2 = gx2 ? gx2 : v.f32(w.gx2), *g1 = gx1 ? gx1 : v.f32(w.gx1);

    // the point that took the maximum, per tile
    if ((r = pointnet::launch_tile(&dgcnn_argmax_kernel, "dgcnn_argmax_kernel", "dgcnn_argmax", kConv3Lds, w.ntiles, B, kPtThreads, st, x2,
                                   n.c3, pooled, v.i32(w.tfirst), N, w.ntiles)) != FX3D_OK) return r;
    HeadBwdArgs hb{};
    hb.tfirst = v.i32(w.tfirst); hb.ntiles = w.ntiles; hb.nc = num_classes; hb.pooled = pooled; hb.glogits = glogits;
    hb.c3 = n.c3; hb.d4 = n.d4; hb.d5 = n.d5; hb.d6 = n.d6; hb.bn4 = n.bn4; hb.bn5 = n.bn5;
    hb.nstar = v.i32(w.nstar); hb.a4 = v.f32(w.a4); hb.a5 = v.f32(w.a5); hb.g5 = v.f32(w.d5); hb.g4 = v.f32(w.d4);
    hb.d3 = v.f32(w.d3); hb.dz3 = v.f32(w.dz3);
    {
        ProfileScope prof("dgcnn_head_bwd", st);
        hipLaunchKernelGGL(dgcnn_head_bwd_kernel, dim3(B), dim3(kHeadThreads), 0, st, hb);
        FX3D_LAUNCH_CHECK();
    }
    // conv_3: the input gradient and the parameter sums, both gathers
    {
        ProfileScope prof("dgcnn_gx2", st);
        hipLaunchKernelGGL(dgcnn_gx2_kernel, dim3(w.ntiles, B), dim3(kPtThreads), 0, st, hb.nstar, hb.dz3, n.c3.W, g2, N);
        FX3D_LAUNCH_CHECK();
    }
    {
        ProfileScope prof("dgcnn_conv3_pgrad", st);
        hipLaunchKernelGGL(dgcnn_conv3_pgrad_kernel, dim3(kFeat), dim3(256), 0, st, x2, hb.nstar, hb.d3, n.c3,
                           grad_block(gn.c3), N, B);
        FX3D_LAUNCH_CHECK();
    }
    // the head's parameter sums over the clouds, and the families from them
    {
        float *H4 = v.f32(w.sums), *h4 = H4 + (size_t)kFeat * 512, *H5 = h4 + 512, *h5 = H5 + (size_t)512 * 256;
        const DenseSums s4{hb.g4, pooled, kFeat, 512, B, H4, h4}, s5{hb.g5, hb.a4, 512, 256, B, H5, h5},
            s6{glogits, hb.a5, 256, num_classes, B, mut(gn.d6.W), mut(gn.d6.b)};
        const DenseFinish f4{H4, h4, n.d4, n.bn4, kFeat, 512, dense_block(gn.d4, gn.bn4)},
            f5{H5, h5, n.d5, n.bn5, 512, 256, dense_block(gn.d5, gn.bn5)};
        auto blocks = [](long long n) { return dim3((unsigned int)((n + 255) / 256)); };
        ProfileScope prof("dgcnn_dense_pgrad", st);
        for (const DenseSums &q : {s4, s5, s6})
            if ((r = pointnet::launch_dense_sums(q, st)) != FX3D_OK) return r;
        for (const DenseFinish &q : {f4, f5}) {
            hipLaunchKernelGGL(dense_finish_kernel, blocks((long long)(q.nin + 5) * q.nout), dim3(256), 0, st, q);
            FX3D_LAUNCH_CHECK();
        }
    }
    // the two stages: EdgeConv2 on x1 with gout = gx2, then EdgeConv1 on x with gout = gx1
    if ((r = fx3d_edgeconv_grad(n.ec2, kEc2, 3, K, x1, N, B, idx2, x2, g2, mut(gn.ec2), g1, wsb + w.scratch, w.ec2_bytes, s)) != FX3D_OK) return r;
    return fx3d_edgeconv_grad(n.ec1, kEc1, 4, K, x, N, B, idx1, x1, g1, mut(gn.ec1), gx, wsb + w.scratch, w.ec1_bytes, s);
}

}  // extern "C"
