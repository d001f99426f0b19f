// PointNet's adjoint (gfx950): the gradients of sum(glogits . logits) with respect to every parameter of the network and to the
// input points, test mode, Float32.  include/flux3d_hip.h ("PointNet adjoint") states the definition and the order of every
// sum; tests/pointnet_grad_ref.py restates it on the host.
//
// The forward's three rounds run first, into the workspace, with the instantiation of pointnet_points_kernel that also writes,
// per (tile of 64 points, channel), the first point that equals the tile's maximum and what the last BatchNorm was given there
// (conv_final_win, pointnet_net.h: the values are still in the accumulators when the maximum is known, so no round is computed
// a second time to find its winners).  Each round keeps its own per-tile maxima.  Then, round by round from the last to the first
// (feat, fstn, stn):
//   pointnet_head_bwd_kernel<FEAT>: one block per cloud.  Thread c folds the tile maxima of channel c, takes the first tile whose
//     maximum equals the cloud's -- its first point is n*(c) -- and the head's dense layers are computed again by the forward's
//     own phases (pointnet_net.h), then walked back (transposed_chain), one thread per element.  What the sums over the clouds
//     need goes to the workspace: every layer's input, the gradient at its contraction, and for a BatchNorm the gradient at its
//     output with the normalised value it was given.
//   pointnet_trunk_bwd_kernel<MODE>: one block = 64 points of one cloud, 4 waves, three (64 x 128) LDS images of the forward's row
//     stride.  The tile's layers below the last are computed again with the forward's own functions and tile loads, the relu's output kept beside
//     the BatchNorm's (the mask and dgamma need the former, the next contraction the latter).  The last layer's input gradient
//     is the gather (a wave owns a point, lists its channels with ballots, ascending, and walks the list eight at a time); the rows
//     the winners of this tile gave the last layer go to the workspace for its parameter sums.  The way back through the 64- and 128-channel layers is
//     v_mfma_f32_32x32x2_f32 on the weights as they lie (back_mfma: B operand W[c + cin o], consecutive lanes consecutive c), the
//     parameter sums of a layer the same instruction on the two resident images (hsum_mfma: the contraction runs over the tile's
//     points, two per instruction, ascending); the 3-channel layers, the column sums and (3 x 3) gT are v_fma_f32 chains.  A
//     tile's sums are stored once, into the tile's partial slab.
//   pointnet_conv3_pgrad_kernel: the last layer's parameter sums, one block per output channel, one chain over the clouds.
//   pointnet_reduce_kernel / pointnet_cloud_reduce_kernel: the chains over the tile partials (b ascending, tile ascending; per
//     cloud for gT and gF); block1_finish_kernel: conv_block1's four families; dense_sums_kernel and bn_sums_kernel: the head's.
#include <initializer_list>

#include "pointnet_net.h"

using namespace fx3d;
using namespace fx3d::mlp;
using namespace fx3d::mlp::pointnet;

namespace {

constexpr int kImg = kTile * kLd;
// three images | x (64 x 3) | x T (64 x 3) | the cloud's n* and conv3 gradient (1024 each) | a channel list per wave (1024 each)
constexpr size_t kTrunkLds = (size_t)(3 * kImg + 2 * kTile * 3 + 2 * kFeat + (kPtThreads / 64) * kFeat) * sizeof(float);
static_assert(kTrunkLds <= kMaxLds, "the trunk adjoint's LDS");
static_assert(kTile == FX3D_POINTNET_GRAD_TILE, "the tile of the stated sums");

// ---- the head ------------------------------------------------------------------------------------------------------------------
struct HeadBwdArgs : HeadArgs {  // the forward's head of the round: its layers, the round's tmax; pooled (1024, B), d1's input
    const int32_t *tfirst;  // (1024, ntiles, B)
    const float *tpre;      // (1024, ntiles, B)
    Bn bn3;                 // the BatchNorm of the round's last convolution
    const float *gup;       // FEAT: glogits (n3, B); else the gradient at the transform (K, K, B)
    int32_t *nstar;         // (1024, B): the winning point, -1 where there is none
    float *a1, *a2;           // the inputs of d2, d3: (512, B), (256, B)
    float *dd1, *dd2, *dd3;   // the gradients at the contractions of d1, d2, d3: (512, B), (256, B), (n3, B)
    float *gy1, *xh1;         // FEAT: the gradient at bn1's output and the normalised value it was given, (512, B)
    float *gy2, *xh2;         // the same for bn2, (256, B)
    float *gy3, *xh3, *dc3;   // the same for bn3 at the winner, and the gradient at the last convolution's contraction, (1024, B)
};

template <bool FEAT>
__global__ __launch_bounds__(kHeadThreads) void pointnet_head_bwd_kernel(const HeadBwdArgs a) {
    __shared__ float v0[kFeat], v1[512], v2[256], z1[512], z2[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float m = fold_tile_maxima(a.tmax, a.ntiles, b);
    int first = kNoPoint;
    float pre = 0.0f;
    {
        const size_t at = (size_t)b * a.ntiles * kFeat + tid;
        for (int k = a.ntiles - 1; k >= 0; --k)  // descending: the last assignment is the first tile that equals the maximum
            if (a.tmax[at + (size_t)k * kFeat] == m) {
                first = a.tfirst[at + (size_t)k * kFeat];
                pre = a.tpre[at + (size_t)k * kFeat];
            }
    }
    const bool won = first != kNoPoint;
    v0[tid] = m;
    a.pooled[(size_t)b * kFeat + tid] = m;
    __syncthreads();
    // the forward's head again, phase by phase (pointnet_net.h); r1, r2: the relus' outputs of this thread's elements
    float r1 = 0.0f, r2 = 0.0f;
    if (tid < 512) {
        r1 = head_relu_dense<512>(a.d1, v0);
        v1[tid] = FEAT ? head_bn(a.bn1, r1) : r1;
        a.a1[(size_t)b * 512 + tid] = v1[tid];
    }
    __syncthreads();
    if (tid < 256) {
        r2 = head_relu_dense<256>(a.d2, v1);
        v2[tid] = head_bn(a.bn2, r2);
        a.a2[(size_t)b * 256 + tid] = v2[tid];
    }
    __syncthreads();
    // the gradient at d3's contraction: the classifier's relu passes where the logit is positive; T[i, j] = d3[K i + j]
    float *dd3 = a.dd3 + (size_t)b * a.n3;
    for (int o = tid; o < a.n3; o += kHeadThreads) {
        float d;
        if (FEAT) {
            const float l = relu(head_dense3(a.d3, v2, a.n3, o));
            d = l > 0.0f ? a.gup[(size_t)b * a.n3 + o] : 0.0f;
        } else {
            d = a.gup[(size_t)b * a.n3 + (o / a.K) + (size_t)a.K * (o % a.K)];
        }
        dd3[o] = d;
    }
    __syncthreads();  // the block's dd3 is in memory
    if (tid < 256) {
        float g = 0.0f;  // the chain over d3's outputs, ascending: 16 bytes of the thread's weight row at a time where n3 allows
        if ((a.n3 & 3) == 0) {
            g = transposed_chain(dd3, a.n3, a.d3.W, tid);
        } else {
            const float *w = a.d3.W + (size_t)a.n3 * tid;
            for (int o = 0; o < a.n3; ++o) g = fmaf(dd3[o], w[o], g);
        }
        const float sd = bn_sd(a.bn2, tid);
        const float d = r2 > 0.0f ? (g * a.bn2.g[tid]) / sd : 0.0f;
        a.gy2[(size_t)b * 256 + tid] = g;
        a.xh2[(size_t)b * 256 + tid] = (r2 - a.bn2.m[tid]) / sd;
        a.dd2[(size_t)b * 256 + tid] = d;
        z2[tid] = d;
    }
    __syncthreads();
    if (tid < 512) {
        const float g = transposed_chain(z2, 256, a.d2.W, tid);
        float d;
        if (FEAT) {
            const float sd = bn_sd(a.bn1, tid);
            d = r1 > 0.0f ? (g * a.bn1.g[tid]) / sd : 0.0f;
            a.gy1[(size_t)b * 512 + tid] = g;
            a.xh1[(size_t)b * 512 + tid] = (r1 - a.bn1.m[tid]) / sd;
        } else {
            d = r1 > 0.0f ? g : 0.0f;
        }
        a.dd1[(size_t)b * 512 + tid] = d;
        z1[tid] = d;
    }
    __syncthreads();
    // the maximum over the points, and the last convolution's BatchNorm (FEAT: no relu before it)
    const float gp = transposed_chain(z1, 512, a.d1.W, tid);
    float gy = 0.0f, xh = 0.0f, d = 0.0f;
    if (won) {
        const float sd = bn_sd(a.bn3, tid);
        gy = gp;
        xh = (pre - a.bn3.m[tid]) / sd;
        d = (FEAT || pre > 0.0f) ? (gy * a.bn3.g[tid]) / sd : 0.0f;
    }
    const size_t at = (size_t)b * kFeat + tid;
    a.nstar[at] = won ? first : -1;
    a.gy3[at] = gy;
    a.xh3[at] = xh;
    a.dc3[at] = d;
}

// ---- the trunk -----------------------------------------------------------------------------------------------------------------
// a conv (relu, BatchNorm) layer's partial: W (cin cout) | b | gamma | beta, the parameter buffer's order
constexpr int layer_part(int cin, int cout) { return cin * cout + 3 * cout; }
// the partial slab of a tile, per round (floats)
constexpr int kP0c1 = 0, kP0c2 = kP0c1 + layer_part(3, 64), kPsize0 = kP0c2 + layer_part(64, 128);
constexpr int kP1c1 = 0, kP1c2 = kP1c1 + layer_part(64, 64), kP1b1 = kP1c2 + layer_part(64, 128), kP1gT = kP1b1 + 3 * 64 + 64,
              kPsize1 = kP1gT + 9;                                   // kP1b1: conv_block1's H (3, 64) | h (64)
constexpr int kP2c1 = 0, kP2gF = kP2c1 + layer_part(64, 128), kPsize2 = kP2gF + 4096;
constexpr int kPsizeMax = kPsize1;
static_assert(kPsize1 >= kPsize0 && kPsize1 >= kPsize2, "the widest partial");

struct TrunkArgs {
    const float *x;         // (3, N, B): MODE 0, 1
    const float *h;         // (64, N, B), the forward's: MODE 1, 2
    const float *tf;        // MODE 0, 1: T (3, 3, B); MODE 2: F (64, 64, B)
    Conv c0;                // MODE 1: conv_block1
    Conv c1, c2;            // the round's convolutions below the last (MODE 2: c1 only)
    const float *W3;        // the last convolution's weights (128, 1024)
    const int32_t *nstar;   // (1024, B)
    const float *dc3;       // (1024, B)
    float *awin;            // (128, 1024, B): the last convolution's input at the winners
    float *part;            // (psize, ntiles, B)
    float *ghf;             // (64, N, B): the feat path's gradient at h; written by MODE 2, read by MODE 1
    float *gh;              // MODE 1, optional: (64, N, B), both paths
    float *gxt;             // (3, N, B): written by MODE 1, read by MODE 0
    float *gx;              // MODE 0, optional: (3, N, B)
    int N, ntiles, psize;
};

// out[p][c] = batchnorm(r[p][c]) for the tile's 64 rows and c < C (the forward's epilogue<kReluBn> after its relu)
__device__ __forceinline__ void bn_image(const float *r, float *out, int C, const Bn &bn) {
    for (int i = threadIdx.x; i < kTile * C; i += kPtThreads) {
        const int p = i / C, c = i - p * C;
        out[p * kLd + c] = batchnorm(r[p * kLd + c], bn.g[c], bn.b[c], bn.m[c], bn_sd(bn, c));
    }
}

// The last convolution's input gradient, the gather: g[p][i], i < 128, = the chain over the channels c the point wins, c
// ascending, of fmaf(dc3[c], W3[i, c], acc); +0 for a point that wins nothing and for the rows beyond the cloud.  A wave owns a
// point, a lane the channels i = lane and lane + 64.  The wave first lists the point's channels in `lst` (its own kFeat ints:
// per 64 channels a ballot, a lane that matches writes at the count of the matches below it, so the list ascends), then walks
// the list eight channels at a time, their sixteen loads in flight before the first fmaf; the order of the chain is the list's.
// The row the point gave the last convolution, BatchNorm(r[p]), goes to awin[i, c, b] for every channel c it wins (one writer
// per (c, b): a channel has one winner).
__device__ __forceinline__ void gather_last(float *g, int32_t *lst, const int32_t *ns, const float *dz, const float *__restrict__ W3,
                                            float *awin, const float *r, const Bn &bn, int b, int p0, int nvalid) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    lst += wave * kFeat;
    for (int p = wave; p < kTile; p += kPtThreads / 64) {
        float acc0 = 0.0f, acc1 = 0.0f;
        if (p < nvalid) {  // wave-uniform
            const int n = p0 + p;
            int cnt = 0;
            for (int cc = 0; cc < kFeat; cc += 64) {
                const bool mine = ns[cc + lane] == n;
                const unsigned long long m = __ballot(mine);
                if (mine) lst[cnt + __popcll(m & ((1ull << lane) - 1))] = cc + lane;
                cnt += __popcll(m);
            }
            __builtin_amdgcn_wave_barrier();  // the wave's list is written before it is read (LDS operations of a wave stay in order)
            if (cnt > 0) {
                const float a0 = batchnorm(r[p * kLd + lane], bn.g[lane], bn.b[lane], bn.m[lane], bn_sd(bn, lane));
                const float a1 = batchnorm(r[p * kLd + 64 + lane], bn.g[64 + lane], bn.b[64 + lane], bn.m[64 + lane], bn_sd(bn, 64 + lane));
                for (int k0 = 0; k0 < cnt; k0 += 8) {
                    float d[8], w0[8], w1[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int c = lst[min(k0 + u, cnt - 1)];
                        d[u] = dz[c];
                        w0[u] = W3[(size_t)128 * c + lane];
                        w1[u] = W3[(size_t)128 * c + 64 + lane];
                        if (k0 + u < cnt) {
                            awin[((size_t)b * kFeat + c) * 128 + lane] = a0;
                            awin[((size_t)b * kFeat + c) * 128 + 64 + lane] = a1;
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u)
                        if (k0 + u < cnt) {  // wave-uniform
                            acc0 = fmaf(d[u], w0[u], acc0);
                            acc1 = fmaf(d[u], w1[u], acc1);
                        }
                }
            }
            __builtin_amdgcn_wave_barrier();  // the list is read before the next point's is written
        }
        g[p * kLd + lane] = acc0;
        g[p * kLd + 64 + lane] = acc1;
    }
}

// A conv (relu, BatchNorm) layer's column pass over the tile's valid rows, ascending, thread o < cout: from gy (the gradient at
// the BatchNorm's output, in g) and r (the relu's output)  dbeta += gy;  dgamma = fmaf(gy, (r - mu) / sd, dgamma);
// d = r > 0 ? (gy gamma) / sd : +0, which takes gy's place;  db += d.  Rows beyond the cloud get d = +0.
__device__ __forceinline__ void column_pass(float *g, const float *r, const Bn &bn, int cout, int nvalid, float *part_b) {
    const int o = threadIdx.x;
    if (o >= cout) return;
    const float gam = bn.g[o], mu = bn.m[o], sd = bn_sd(bn, o);
    float sb = 0.0f, sg = 0.0f, sbe = 0.0f;
    for (int p = 0; p < nvalid; ++p) {
        const float gy = g[p * kLd + o], rv = r[p * kLd + o];
        sbe = sbe + gy;
        sg = fmaf(gy, (rv - mu) / sd, sg);
        const float d = rv > 0.0f ? (gy * gam) / sd : 0.0f;
        sb = sb + d;
        g[p * kLd + o] = d;
    }
    for (int p = nvalid; p < kTile; ++p) g[p * kLd + o] = 0.0f;
    part_b[o] = sb;
    part_b[cout + o] = sg;
    part_b[2 * cout + o] = sbe;
}

template <int MODE>
__global__ __launch_bounds__(kPtThreads) void pointnet_trunk_bwd_kernel(const TrunkArgs a) {
    extern __shared__ float lds[];
    float *I0 = lds, *I1 = lds + kImg, *I2 = lds + 2 * kImg, *xs = lds + 3 * kImg, *xt = xs + kTile * 3;
    int32_t *ns = reinterpret_cast<int32_t *>(xt + kTile * 3);
    float *dzs = reinterpret_cast<float *>(ns + kFeat);
    int32_t *lst = reinterpret_cast<int32_t *>(dzs + kFeat);  // a list of kFeat channels per wave (gather_last)
    const int tile = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int p0 = tile * kTile;
    const int nvalid = min(kTile, a.N - p0);
    float *part = a.part + ((size_t)b * a.ntiles + tile) * a.psize;
    for (int c = tid; c < kFeat; c += kPtThreads) {
        ns[c] = a.nstar[(size_t)b * kFeat + c];
        dzs[c] = a.dc3[(size_t)b * kFeat + c];
    }
    if (MODE != 2) load_xs(xs, a.x, b, a.N, p0, nvalid);
    if (MODE == 1) load_tile64(I2, a.h, b, a.N, p0, nvalid);
    if (MODE == 2) load_tile64(I0, a.h, b, a.N, p0, nvalid);
    __syncthreads();

    if (MODE == 2) {
        // forward: h F in I0[64..], r1 = relu(conv1) in I1
        conv_mfma<64, kNone, false>(I0, I0 + 64, 64, a.tf + (size_t)b * 4096, nullptr, Bn{}, nvalid, nullptr);
        __syncthreads();
        conv_mfma<64, kRelu, false>(I0 + 64, I1, 128, a.c1.W, a.c1.b, a.c1.bn, nvalid, nullptr);
        __syncthreads();
        gather_last(I2, lst, ns, dzs, a.W3, a.awin, I1, a.c1.bn, b, p0, nvalid);
        __syncthreads();
        column_pass(I2, I1, a.c1.bn, 128, nvalid, part + kP2c1 + 64 * 128);
        __syncthreads();
        hsum_mfma(I0 + 64, I2, 64, 128, part + kP2c1);
        back_mfma<128>(I2, I1, 64, a.c1.W);  // the gradient at h F, in r1's place
        __syncthreads();
        hsum_mfma(I0, I1, 64, 64, part + kP2gF);                    // gF[i, j] = sum_n h[i, n] g[j, n]
        back_mfma<64>(I1, I1 + 64, 64, a.tf + (size_t)b * 4096);   // the feat path into h: the chain over j of g[j] F[i, j]
        __syncthreads();
        float *gb = a.ghf + ((size_t)b * a.N + p0) * 64;
        for (int i = tid; i < nvalid * 64; i += kPtThreads) gb[i] = I1[(i >> 6) * kLd + 64 + (i & 63)];
        return;
    }

    // MODE 0, 1 forward: r1 in I0[0..63], a1 = BN(r1) in I0[64..127], r2 in I1
    if (MODE == 0) {
        conv3<kRelu>(xs, I0, kLd, 64, a.c1.W, a.c1.b, a.c1.bn);
    } else {
        conv3<kNone>(xs, xt, 3, 3, a.tf + (size_t)b * 9, nullptr, Bn{});
        conv_mfma<64, kRelu, false>(I2, I0, 64, a.c1.W, a.c1.b, a.c1.bn, nvalid, nullptr);
    }
    __syncthreads();
    bn_image(I0, I0 + 64, 64, a.c1.bn);
    __syncthreads();
    conv_mfma<64, kRelu, false>(I0 + 64, I1, 128, a.c2.W, a.c2.b, a.c2.bn, nvalid, nullptr);
    __syncthreads();
    gather_last(I2, lst, ns, dzs, a.W3, a.awin, I1, a.c2.bn, b, p0, nvalid);
    __syncthreads();
    constexpr int c2at = MODE == 0 ? kP0c2 : kP1c2, c1at = MODE == 0 ? kP0c1 : kP1c1, c1in = MODE == 0 ? 3 : 64;
    column_pass(I2, I1, a.c2.bn, 128, nvalid, part + c2at + 64 * 128);
    __syncthreads();
    hsum_mfma(I0 + 64, I2, 64, 128, part + c2at);
    back_mfma<128>(I2, I1, 64, a.c2.W);  // the gradient at a1, in r2's place
    __syncthreads();
    column_pass(I1, I0, a.c1.bn, 64, nvalid, part + c1at + c1in * 64);
    if (MODE == 1) load_tile64(I1 + 64, a.h, b, a.N, p0, nvalid);  // h again, beside dz1
    __syncthreads();

    if (MODE == 0) {
        hsum3(xs, I1, nvalid, 0, part + kP0c1);
        if (a.gx != nullptr && tid < kTile * 3) {
            const int p = tid / 3, i = tid - 3 * p;
            if (p < nvalid) {
                float sp = 0.0f, tp = 0.0f;  // the stn path: the chain over conv1's outputs; the path through T: over j
                for (int o = 0; o < 64; ++o) sp = fmaf(I1[p * kLd + o], a.c1.W[i + 3 * o], sp);
                const float *g = a.gxt + ((size_t)b * a.N + p0 + p) * 3, *T = a.tf + (size_t)b * 9;
                for (int j = 0; j < 3; ++j) tp = fmaf(g[j], T[i + 3 * j], tp);
                a.gx[((size_t)b * a.N + p0 + p) * 3 + i] = tp + sp;
            }
        }
        return;
    }

    // MODE 1: fstn's conv1, then both paths into h, conv_block1 and the input transform
    hsum_mfma(I1 + 64, I1, 64, 64, part + kP1c1);
    back_mfma<64>(I1, I2, 64, a.c1.W);  // the fstn path into h, in dz2's place
    __syncthreads();
    {
        const float *gf = a.ghf + ((size_t)b * a.N + p0) * 64;
        float *go = a.gh ? a.gh + ((size_t)b * a.N + p0) * 64 : nullptr;
        for (int i = tid; i < kTile * 64; i += kPtThreads) {
            const int at = (i >> 6) * kLd + (i & 63);
            float d = 0.0f;
            if (i < nvalid * 64) {
                const float g = gf[i] + I2[at];  // the feat path + the fstn path
                if (go) go[i] = g;
                d = I1[at + 64] > 0.0f ? g : 0.0f;  // conv_block1: BatchNorm, then relu
            }
            I2[at] = d;
        }
    }
    __syncthreads();
    if (tid < 64) {  // h0[o] = sum of d0 over the tile's valid rows
        float acc = 0.0f;
        for (int p = 0; p < nvalid; ++p) acc = acc + I2[p * kLd + tid];
        part[kP1b1 + 192 + tid] = acc;
    }
    hsum3(xt, I2, nvalid, 64, part + kP1b1);
    // the gradient at x T: the chain over conv_block1's outputs of dz0 = (d0 gamma) / sd; also into I0[0..2], for gT
    if (tid < kTile * 3) {
        const int p = tid / 3, j = tid - 3 * p;
        float acc = 0.0f;
        if (p < nvalid) {
            for (int o = 0; o < 64; ++o)
                acc = fmaf((I2[p * kLd + o] * a.c0.bn.g[o]) / bn_sd(a.c0.bn, o), a.c0.W[j + 3 * o], acc);
            a.gxt[((size_t)b * a.N + p0 + p) * 3 + j] = acc;
        }
        I0[p * kLd + j] = acc;  // (r1 is consumed; the threads beside this one read I2 and xt)
    }
    __syncthreads();
    if (tid < 9) {  // gT[i, j] = sum_n x[i, n] gxt[j, n] over the tile's valid rows
        const int i = tid % 3, j = tid / 3;
        float acc = 0.0f;
        for (int p = 0; p < nvalid; ++p) acc = fmaf(xs[p * 3 + i], I0[p * kLd + j], acc);
        part[kP1gT + tid] = acc;
    }
}

// ---- the last convolution's parameter sums -----------------------------------------------------------------------------------------
// one block per output channel c, thread i owns dW[i, c]: one chain over the clouds that have a winner, b ascending
__global__ __launch_bounds__(128) void pointnet_conv3_pgrad_kernel(const float *__restrict__ awin, const int32_t *__restrict__ nstar,
                                                                   const float *__restrict__ dc3, const float *__restrict__ gy3,
                                                                   const float *__restrict__ xh3, const GradBlock g, int B) {
    const int c = blockIdx.x, i = threadIdx.x;
    float H = 0.0f, sb = 0.0f, sg = 0.0f, sbe = 0.0f;
    for (int b = 0; b < B; ++b) {
        const size_t at = (size_t)b * kFeat + c;
        if (nstar[at] < 0) continue;  // block-uniform
        const float d = dc3[at], gy = gy3[at];
        H = fmaf(awin[at * 128 + i], d, H);
        sb = sb + d;
        sbe = sbe + gy;
        sg = fmaf(gy, xh3[at], sg);
    }
    g.W[i + (size_t)128 * c] = H;
    if (i == 0) {
        g.b[c] = sb;
        g.g[c] = sg;
        g.be[c] = sbe;
        g.m[c] = 0.0f;
        g.v[c] = 0.0f;
    }
}

// ---- the finishing kernels -----------------------------------------------------------------------------------------------------
// dst[e] = the chain of Float32 additions from +0 over the tile partials (b ascending, tile ascending) for e < n; +0 for the nz
// elements after them (a BatchNorm's mu and var).  blockIdx.y: the segment.
__global__ __launch_bounds__(256) void pointnet_reduce_kernel(const ReduceArgs a) {
    const Seg s = blockIdx.y == 0 ? a.s[0] : blockIdx.y == 1 ? a.s[1] : a.s[2];
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= s.n + s.nz) return;
    float acc = 0.0f;
    if (e < s.n) {
        const float *p = a.part + s.at + e;
#pragma unroll 8
        for (int q = 0; q < a.nparts; ++q) acc = acc + p[(size_t)q * a.psize];  // (the loads of 8 steps in flight)
    }
    s.dst[e] = acc;
}

// the same per cloud (gT, gF): dst[e + n b] = the chain over the cloud's tiles, ascending
__global__ __launch_bounds__(256) void pointnet_cloud_reduce_kernel(const float *__restrict__ part, int psize, int at, int ntiles, int n,
                                                                    float *__restrict__ dst) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (e >= n) return;
    float acc = 0.0f;
    for (int t = 0; t < ntiles; ++t) acc = acc + part[((size_t)b * ntiles + t) * psize + at + e];
    dst[e + (size_t)n * b] = acc;
}

// conv_block1 (BatchNorm, then relu): "EdgeConv parameter adjoint"'s four families from H (3, 64) | h (64) in sums
__global__ __launch_bounds__(256) void block1_finish_kernel(const float *__restrict__ sums, const Conv c, const GradBlock g) {
    const int e = threadIdx.x;
    const float *H = sums, *h = sums + 192;
    if (e < 192) {
        const int o = e / 3;
        g.W[e] = (H[e] * c.bn.g[o]) / bn_sd(c.bn, o);
        return;
    }
    const int o = e - 192;
    const float sd = bn_sd(c.bn, o);
    float acc = 0.0f;
    for (int i = 0; i < 3; ++i) acc = fmaf(c.W[i + 3 * o], H[i + 3 * o], acc);
    g.b[o] = (h[o] * c.bn.g[o]) / sd;
    g.g[o] = (acc + (c.b[o] - c.bn.m[o]) * h[o]) / sd;
    g.be[o] = h[o];
    g.m[o] = 0.0f;
    g.v[o] = 0.0f;
}

__global__ __launch_bounds__(256) void dense_sums_kernel(const DenseSums s) {
    dense_sums(s, (long long)blockIdx.x * blockDim.x + threadIdx.x);
}

// a head BatchNorm's sums over the clouds, b ascending: dbeta[o] = sum gy[o, b], dgamma[o] = fmaf(gy[o, b], xh[o, b], acc); mu, var: +0
__global__ __launch_bounds__(256) void bn_sums_kernel(const float *__restrict__ gy, const float *__restrict__ xh, int n, int B,
                                                      const GradBlock g) {
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= n) return;
    float sg = 0.0f, sbe = 0.0f;
    for (int b = 0; b < B; ++b) {
        sbe = sbe + gy[o + (size_t)n * b];
        sg = fmaf(gy[o + (size_t)n * b], xh[o + (size_t)n * b], sg);
    }
    g.g[o] = sg;
    g.be[o] = sbe;
    g.m[o] = 0.0f;
    g.v[o] = 0.0f;
}

// The workspace: the forward's h, T, F and per round the tile maxima, first points and BatchNorm inputs | the head's vectors
// (used by the rounds in turn) | the winners' rows | the tile partials (the widest round's) | conv_block1's sums | the feat
// path's gradient at h | gxt, gT, gF (used where the caller gives none)
struct GradWs {
    size_t h, T, F, tmax[3], tfirst[3], tpre[3];
    size_t nstar, pooled, a1, a2, dd1, dd2, dd3, gy1, xh1, gy2, xh2, gy3, xh3, dc3;
    size_t awin, part, sums, ghf, gxt, gT, gF, total;
    int ntiles;
};
GradWs grad_ws(int N, int B, int nc) {
    GradWs w;
    w.ntiles = (N + kTile - 1) / kTile;
    const size_t f = sizeof(float), nb = (size_t)N * B, tb = (size_t)kFeat * w.ntiles * B;
    WsBump ws;
    w.h = ws.put(64 * nb * f);
    w.T = ws.put((size_t)9 * B * f);
    w.F = ws.put((size_t)4096 * B * f);
    for (int r = 0; r < 3; ++r) {
        w.tmax[r] = ws.put(tb * f);
        w.tfirst[r] = ws.put(tb * sizeof(int32_t));
        w.tpre[r] = ws.put(tb * f);
    }
    w.nstar = ws.put((size_t)kFeat * B * sizeof(int32_t));
    w.pooled = ws.put((size_t)kFeat * B * f);
    w.a1 = ws.put((size_t)512 * B * f);
    w.a2 = ws.put((size_t)256 * B * f);
    w.dd1 = ws.put((size_t)512 * B * f);
    w.dd2 = ws.put((size_t)256 * B * f);
    w.dd3 = ws.put((size_t)(nc > 4096 ? nc : 4096) * B * f);
    w.gy1 = ws.put((size_t)512 * B * f);
    w.xh1 = ws.put((size_t)512 * B * f);
    w.gy2 = ws.put((size_t)256 * B * f);
    w.xh2 = ws.put((size_t)256 * B * f);
    w.gy3 = ws.put((size_t)kFeat * B * f);
    w.xh3 = ws.put((size_t)kFeat * B * f);
    w.dc3 = ws.put((size_t)kFeat * B * f);
    w.awin = ws.put((size_t)128 * kFeat * B * f);
    w.part = ws.put((size_t)kPsizeMax * w.ntiles * B * f);
    w.sums = ws.put((size_t)256 * f);
    w.ghf = ws.put(64 * nb * f);
    w.gxt = ws.put(3 * nb * f);
    w.gT = ws.put((size_t)9 * B * f);
    w.gF = ws.put((size_t)4096 * B * f);
    w.total = ws.at;
    return w;
}

dim3 blocks(long long n) { return dim3((unsigned int)((n + 255) / 256)); }

template <bool FEAT>
fx3d_status launch_head_bwd(const HeadBwdArgs &a, int B, hipStream_t st) {
    ProfileScope prof("pointnet_head_bwd", st);
    hipLaunchKernelGGL(pointnet_head_bwd_kernel<FEAT>, dim3(B), dim3(kHeadThreads), 0, st, a);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

template <int MODE>
fx3d_status launch_trunk(const TrunkArgs &a, int B, hipStream_t st) {
    const fx3d_status rc = ensure_dynamic_lds(reinterpret_cast<const void *>(&pointnet_trunk_bwd_kernel<MODE>), (int)kTrunkLds,
                                              "pointnet_trunk_bwd_kernel");
    if (rc != FX3D_OK) return rc;
    ProfileScope prof("pointnet_trunk_bwd", st);
    hipLaunchKernelGGL(pointnet_trunk_bwd_kernel<MODE>, dim3(a.ntiles, B), dim3(kPtThreads), kTrunkLds, st, a);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

// a conv (relu, BatchNorm) layer's segment of a tile partial: W | b | gamma | beta summed, mu | var zeroed
Seg layer_seg(int at, const Conv &g, int cin, int cout) { return Seg{at, mut(g.W), layer_part(cin, cout), 2 * cout}; }

}  // namespace

namespace fx3d {
namespace mlp {
namespace pointnet {

fx3d_status launch_reduce(const ReduceArgs &ra, int nsegs, hipStream_t st) {
    int widest = 0;
    for (int k = 0; k < nsegs; ++k) widest = ra.s[k].n + ra.s[k].nz > widest ? ra.s[k].n + ra.s[k].nz : widest;
    hipLaunchKernelGGL(pointnet_reduce_kernel, dim3(blocks(widest).x, nsegs), dim3(256), 0, st, ra);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

fx3d_status launch_cloud_reduce(const float *part, int psize, int at, int ntiles, int n, int B, float *dst, hipStream_t st) {
    hipLaunchKernelGGL(pointnet_cloud_reduce_kernel, dim3(blocks(n).x, B), dim3(256), 0, st, part, psize, at, ntiles, n, dst);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

fx3d_status launch_dense_sums(const DenseSums &q, hipStream_t st) {
    hipLaunchKernelGGL(dense_sums_kernel, blocks((long long)(q.nin + 1) * q.nout), dim3(256), 0, st, q);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

}  // namespace pointnet
}  // namespace mlp
}  // namespace fx3d

extern "C" {

fx3d_status fx3d_pointnet_grad_workspace_bytes(int32_t N, int32_t B, int32_t num_classes, size_t *bytes) {
    FX3D_REQUIRE(bytes != nullptr, "fx3d_pointnet_grad_workspace_bytes: bytes is NULL");
    const fx3d_status rc = check_sizes("fx3d_pointnet_grad_workspace_bytes", N, B, num_classes);
    if (rc != FX3D_OK) return rc;
    *bytes = grad_ws(N, B, num_classes).total;
    return FX3D_OK;
}

fx3d_status fx3d_pointnet_grad(const float *params_dev, int32_t num_classes, const float *x, int32_t N, int32_t B,
                               const float *glogits, float *gparams, float *gx, float *gstn, float *gfstn, float *gh, float *gxt,
                               void *ws, size_t ws_bytes, fx3d_stream_t s) {
    const char *fn = "fx3d_pointnet_grad";
    FX3D_REQUIRE(params_dev && x && glogits && gparams && ws, "%s: params_dev, x, glogits, gparams and ws must not be NULL", fn);
    fx3d_status r = check_sizes(fn, N, B, num_classes);
    if (r != FX3D_OK) return r;
    const GradWs w = grad_ws(N, B, num_classes);
    FX3D_REQUIRE(ws_bytes >= w.total, "%s: workspace of %zu bytes, fx3d_pointnet_grad_workspace_bytes says %zu", fn, ws_bytes, w.total);
    FX3D_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "%s: ws must be 256-byte aligned", fn);
    const Net n = layout(params_dev, num_classes), gn = layout(gparams, num_classes);
    hipStream_t st = as_stream(s);
    const WsView v{static_cast<char *>(ws)};
    float *T = v.f32(w.T), *F = v.f32(w.F), *gT = gstn ? gstn : v.f32(w.gT), *gF = gfstn ? gfstn : v.f32(w.gF);
    float *gxt_ = gxt ? gxt : v.f32(w.gxt);
    const int nt = w.ntiles;

    // the forward's three rounds, each with its winners per tile; the classifier's head is computed in the head adjoint
    {
        PointArgs p{};
        p.x = x; p.h = v.f32(w.h); p.N = N; p.ntiles = nt;
        for (int mode = 0; mode < 3; ++mode) {
            set_round(p, n, mode, T, F);
            p.tmax = v.f32(w.tmax[mode]); p.tfirst = v.i32(w.tfirst[mode]); p.tpre = v.f32(w.tpre[mode]);
            if ((r = launch_points(mode, true, p, B, st)) != FX3D_OK) return r;
            if (mode < 2 && (r = launch_head(false, stn_head(n, mode, p.tmax, nt, T, F, nullptr), B, st)) != FX3D_OK) return r;
        }
    }

    HeadBwdArgs hb{};
    hb.nstar = v.i32(w.nstar); hb.a1 = v.f32(w.a1); hb.a2 = v.f32(w.a2);
    hb.dd1 = v.f32(w.dd1); hb.dd2 = v.f32(w.dd2); hb.dd3 = v.f32(w.dd3);
    hb.gy1 = v.f32(w.gy1); hb.xh1 = v.f32(w.xh1); hb.gy2 = v.f32(w.gy2); hb.xh2 = v.f32(w.xh2);
    hb.gy3 = v.f32(w.gy3); hb.xh3 = v.f32(w.xh3); hb.dc3 = v.f32(w.dc3);
    // round k's head as the forward has it, over the layers of net (the parameters, or their gradients); for the adjoint also
    // the round's winners, the BatchNorm of its last convolution and the gradient that arrives
    auto head_of = [&](const Net &net, int k) {
        const float *tmax = v.f32(w.tmax[k]);
        return k == 2 ? feat_head(net, num_classes, tmax, nt, nullptr, nullptr, nullptr) : stn_head(net, k, tmax, nt, T, F, nullptr);
    };
    auto head_round = [&](int k, const Bn &bn3, const float *gup) {
        static_cast<HeadArgs &>(hb) = head_of(n, k);
        hb.pooled = v.f32(w.pooled); hb.tfirst = v.i32(w.tfirst[k]); hb.tpre = v.f32(w.tpre[k]); hb.bn3 = bn3; hb.gup = gup;
    };

    TrunkArgs t{};
    t.x = x; t.h = v.f32(w.h); t.nstar = hb.nstar; t.dc3 = hb.dc3; t.awin = v.f32(w.awin); t.part = v.f32(w.part);
    t.ghf = v.f32(w.ghf); t.gh = gh; t.gxt = gxt_; t.gx = gx; t.N = N; t.ntiles = nt;

    // the last convolution's sums, the head's sums over the clouds, and the chains over the tile partials of one round
    auto conv3_sums = [&](const Conv &g3) -> fx3d_status {
        ProfileScope prof("pointnet_conv3_pgrad", st);
        hipLaunchKernelGGL(pointnet_conv3_pgrad_kernel, dim3(kFeat), dim3(128), 0, st, t.awin, hb.nstar, hb.dc3, hb.gy3, hb.xh3,
                           grad_block(g3), B);
        FX3D_LAUNCH_CHECK();
        return FX3D_OK;
    };
    auto head_sums = [&](int k) -> fx3d_status {
        ProfileScope prof("pointnet_head_pgrad", st);
        const HeadArgs g = head_of(gn, k);
        const DenseSums s1{hb.dd1, hb.pooled, kFeat, 512, B, mut(g.d1.W), mut(g.d1.b)}, s2{hb.dd2, hb.a1, 512, 256, B, mut(g.d2.W), mut(g.d2.b)},
            s3{hb.dd3, hb.a2, 256, g.n3, B, mut(g.d3.W), mut(g.d3.b)};
        for (const DenseSums &q : {s1, s2, s3}) {
            if ((r = launch_dense_sums(q, st)) != FX3D_OK) return r;
        }
        if (k == 2) {
            hipLaunchKernelGGL(bn_sums_kernel, blocks(512), dim3(256), 0, st, hb.gy1, hb.xh1, 512, B, grad_block(g.bn1));
            FX3D_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(bn_sums_kernel, blocks(256), dim3(256), 0, st, hb.gy2, hb.xh2, 256, B, grad_block(g.bn2));
        FX3D_LAUNCH_CHECK();
        return FX3D_OK;
    };
    auto reduce = [&](std::initializer_list<Seg> segs, int psize) -> fx3d_status {
        ReduceArgs ra{};
        ra.part = t.part; ra.psize = psize; ra.nparts = nt * B;
        int k = 0;
        for (const Seg &q : segs) ra.s[k++] = q;
        return launch_reduce(ra, k, st);
    };
    auto cloud_reduce = [&](int psize, int at, int cnt, float *dst) -> fx3d_status {
        return launch_cloud_reduce(t.part, psize, at, nt, cnt, B, dst, st);
    };

    // feat and cls
    head_round(2, n.f2.bn, glogits);
    if ((r = launch_head_bwd<true>(hb, B, st)) != FX3D_OK) return r;
    t.tf = F; t.c1 = n.f1; t.W3 = n.f2.W; t.psize = kPsize2;
    if ((r = launch_trunk<2>(t, B, st)) != FX3D_OK) return r;
    if ((r = conv3_sums(gn.f2)) != FX3D_OK) return r;
    if ((r = head_sums(2)) != FX3D_OK) return r;
    {
        ProfileScope prof("pointnet_grad_reduce", st);
        if ((r = reduce({layer_seg(kP2c1, gn.f1, 64, 128)}, kPsize2)) != FX3D_OK) return r;
        if ((r = cloud_reduce(kPsize2, kP2gF, 4096, gF)) != FX3D_OK) return r;
    }

    // fstn, conv_block1 and the input transform
    head_round(1, n.fstn.c3.bn, gF);
    if ((r = launch_head_bwd<false>(hb, B, st)) != FX3D_OK) return r;
    t.tf = T; t.c0 = n.block1; t.c1 = n.fstn.c1; t.c2 = n.fstn.c2; t.W3 = n.fstn.c3.W; t.psize = kPsize1;
    if ((r = launch_trunk<1>(t, B, st)) != FX3D_OK) return r;
    if ((r = conv3_sums(gn.fstn.c3)) != FX3D_OK) return r;
    if ((r = head_sums(1)) != FX3D_OK) return r;
    {
        ProfileScope prof("pointnet_grad_reduce", st);
        if ((r = reduce({layer_seg(kP1c1, gn.fstn.c1, 64, 64), layer_seg(kP1c2, gn.fstn.c2, 64, 128), Seg{kP1b1, v.f32(w.sums), 256, 0}},
                        kPsize1)) != FX3D_OK) return r;
        hipLaunchKernelGGL(block1_finish_kernel, dim3(1), dim3(256), 0, st, v.f32(w.sums), n.block1, grad_block(gn.block1));
        FX3D_LAUNCH_CHECK();
        if ((r = cloud_reduce(kPsize1, kP1gT, 9, gT)) != FX3D_OK) return r;
    }

    // stn, and the two paths into x
    head_round(0, n.stn.c3.bn, gT);
    if ((r = launch_head_bwd<false>(hb, B, st)) != FX3D_OK) return r;
    t.c1 = n.stn.c1; t.c2 = n.stn.c2; t.W3 = n.stn.c3.W; t.psize = kPsize0;
    if ((r = launch_trunk<0>(t, B, st)) != FX3D_OK) return r;
    if ((r = conv3_sums(gn.stn.c3)) != FX3D_OK) return r;
    if ((r = head_sums(0)) != FX3D_OK) return r;
    ProfileScope prof("pointnet_grad_reduce", st);
    return reduce({layer_seg(kP0c1, gn.stn.c1, 3, 64), layer_seg(kP0c2, gn.stn.c2, 64, 128)}, kPsize0);
}

}  // extern "C"
