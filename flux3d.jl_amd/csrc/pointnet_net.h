// What pointnet.hip (the forward), pointnet_train.hip (the training-mode forward), pointnet_grad.hip (the adjoint) and
// pointnet_grad_train.hip (the training-mode adjoint) share.  At the end, what only some of them share: the fold of a BatchNorm's
// Float64 tile sums (the two training-mode units) and a BatchNorm's batch statistics (pointnet_train.hip, and with it the
// training-mode forwards of DGCNN and EdgeConv), and the adjoints' MFMA chains over a tile (hsum_mfma, back_mfma, hsum3) with the
// launches of pointnet_grad.hip's finishing kernels; and what the training-mode adjoints of PointNet and DGCNN share (bn_gv, BnOut,
// LastChannel, the cloud-sums launch, and the dense adjoint of the 1024-output convolution under a maximum: last_back, last_pgrad,
// their arguments and launch_tile).
// stnkd.hip, stnKD(K) as a layer of its own, is round_trunk's MODE 3 on these kernels: it adds a host walk, no trunk of its own.
// On the host: the walk over the flat parameter buffer, the forward's workspace, the size check of the entries, the
// arguments of the forward's two kernels per round (set_round, stn_head, feat_head) and their launches (defined in
// pointnet.hip, which owns the kernels).  On the device: a round's layer chain (round_trunk, with its tile loads), the slab
// walk with an epilogue on the accumulators (for_each_slab; conv_final_win, the last layer with the winners the adjoint
// needs, is one body of it) and the head's phases (head_pool .. head_finish).
#pragma once
#include <climits>

#include "mlp_common.h"

namespace fx3d {
namespace mlp {
namespace pointnet {  // (dgcnn_net.h has a Net of its own)

constexpr size_t kPtLds = (size_t)(2 * kTile * kLd + 2 * kTile * 3) * sizeof(float);
constexpr int kNoPoint = INT_MAX;  // a tile in which no point reproduces its maximum (a NaN maximum)

struct PointArgs {
    const float *x;   // (3, N, B): MODE 0, 1; (K, N, B): MODE 3
    float *h;         // workspace (64, N, B): written by MODE 1, read by MODE 2
    const float *tf;  // the cloud's transform, (3, 3, B) for MODE 1, (64, 64, B) for MODE 2
    Conv c0;          // MODE 1: conv_block1
    Conv c1, c2, c3;  // the round's convolutions (MODE 2: c2, c3)
    float *tmax;      // (1024, ntiles, B)
    int N, ntiles;
    int32_t *tfirst;  // the adjoint's launches (WIN): (1024, ntiles, B), the first point of the tile that equals the tile's maximum
    float *tpre;      //   and what the last layer's BatchNorm was given at that point
    int K;            // MODE 3: the channels of x, 1 .. 128
};

struct HeadArgs {
    const float *tmax;  // (1024, ntiles, B)
    int ntiles;
    Dense d1, d2, d3;   // 1024 -> 512, 512 -> 256, 256 -> n3
    Bn bn1, bn2;        // FEAT: BatchNorm(512) after d1; both: BatchNorm(256) after d2
    int n3, K;          // outputs of d3; stn / fstn: n3 = K K
    float *mat, *mat_user;  // stn / fstn: (K, K, B) in the workspace and, optionally, the caller's copy
    float *pooled;          // FEAT, optional: (1024, B)
    float *logits, *probs;  // FEAT: (n3, B) each; logits is the caller's array or the workspace
};

struct Stn { Conv c1, c2, c3; Dense d1, d2, d3; Bn bn; };
struct Net {
    Stn stn, fstn;
    Conv block1, f1, f2;
    Dense fd1, fd2, cls;
    Bn fbn1, fbn2;
    long long count;
};

inline Stn layout_stn(Cursor &c, int K) {
    Stn s;
    s.c1 = c.conv(K, 64);     s.c1.bn = c.bn(64);
    s.c2 = c.conv(64, 128);   s.c2.bn = c.bn(128);
    s.c3 = c.conv(128, 1024); s.c3.bn = c.bn(1024);
    s.d1 = c.dense(1024, 512);
    s.d2 = c.dense(512, 256);
    s.bn = c.bn(256);
    s.d3 = c.dense(256, K * K);
    return s;
}

inline Net layout(const float *params, int num_classes) {
    Cursor c{params, 0};
    Net n;
    n.stn = layout_stn(c, 3);
    n.block1 = c.conv(3, 64);   n.block1.bn = c.bn(64);
    n.fstn = layout_stn(c, 64);
    n.f1 = c.conv(64, 128);     n.f1.bn = c.bn(128);
    n.f2 = c.conv(128, 1024);   n.f2.bn = c.bn(1024);
    n.fd1 = c.dense(1024, 512); n.fbn1 = c.bn(512);
    n.fd2 = c.dense(512, 256);  n.fbn2 = c.bn(256);
    n.cls = c.dense(256, num_classes);
    n.count = c.at;
    return n;
}

// ---- training mode (pointnet_train.hip): the 13 BatchNorms in forward order -- stn.bn1 .. bn4, conv_block1.bn, fstn.bn1 .. bn4,
// feat.bn1 .. bn4 -- which is the order of their mu / sigma2 slots in the flat parameter buffer and of the statistics buffer
// (flux3d_hip.h "PointNet training-mode forward": per BatchNorm mean (C) then variance (C)).  f(bn, C) for each of them.
constexpr int kNumBn = 13;
constexpr int kStatChannels = 2 * (64 + 128 + kFeat + 256) + 64 + 128 + kFeat + 512 + 256;  // 4928
template <class NetT, class F>
inline void for_each_bn(NetT &n, F f) {
    auto stn = [&](auto &s) { f(s.c1.bn, 64); f(s.c2.bn, 128); f(s.c3.bn, kFeat); f(s.bn, 256); };
    stn(n.stn);
    f(n.block1.bn, 64);
    stn(n.fstn);
    f(n.f1.bn, 128); f(n.f2.bn, kFeat); f(n.fbn1, 512); f(n.fbn2, 256);
}
// the network whose BatchNorms read their mean and variance from a statistics buffer instead of the running values: the
// test-mode kernels then evaluate every layer whose statistics are there in training mode
inline Net with_batch_stats(Net n, const float *stats) {
    size_t at = 0;
    for_each_bn(n, [&](Bn &bn, int C) {
        bn.m = stats + at;
        bn.v = stats + at + C;
        at += 2 * (size_t)C;
    });
    return n;
}

// the workspace: h (64, N, B) | per-tile maxima (1024, ntiles, B) | T (3, 3, B) | F (64, 64, B) | logits (num_classes, B)
struct WsPlan { size_t h, tmax, T, F, logits, total; int ntiles; };
inline WsPlan ws_plan(int N, int B, int nc) {
    WsPlan w;
    w.ntiles = (N + kTile - 1) / kTile;
    WsBump ws;
    w.h = ws.put((size_t)64 * N * B * sizeof(float));
    w.tmax = ws.put((size_t)kFeat * w.ntiles * B * sizeof(float));
    w.T = ws.put((size_t)9 * B * sizeof(float));
    w.F = ws.put((size_t)4096 * B * sizeof(float));
    w.logits = ws.put((size_t)nc * B * sizeof(float));
    w.total = ws.at;
    return w;
}

inline fx3d_status check_sizes(const char *fn, int32_t N, int32_t B, int32_t nc) {
    FX3D_REQUIRE(nc >= 1 && nc <= (1 << 20), "%s: num_classes must be in [1, 2^20], got %d", fn, nc);
    FX3D_REQUIRE(N >= 1 && B >= 1, "%s: N and B must be positive, got N=%d B=%d", fn, N, B);
    FX3D_REQUIRE(B <= 65535, "%s: B must be at most 65535, got %d", fn, B);
    FX3D_REQUIRE((long long)N * B <= (1ll << 31), "%s: N * B must be at most 2^31, got %lld", fn, (long long)N * B);
    return FX3D_OK;
}

// a workspace as typed arrays at the offsets of its plan
struct WsView {
    char *base;
    float *f32(size_t at) const { return reinterpret_cast<float *>(base + at); }
    int32_t *i32(size_t at) const { return reinterpret_cast<int32_t *>(base + at); }
    double *f64(size_t at) const { return reinterpret_cast<double *>(base + at); }
};

// ---- the three rounds, mode 0 = stn, 1 = fstn, 2 = feat: what each gives the forward's two kernels ----------------------------
// the round's convolutions and the transform in front of them: stn reads x; fstn x T, through conv_block1 (kept as h); feat h F
inline void set_round(PointArgs &p, const Net &n, int mode, const float *T, const float *F) {
    const Stn &s = mode == 0 ? n.stn : n.fstn;
    p.tf = mode == 0 ? nullptr : mode == 1 ? T : F;
    p.c0 = n.block1;
    p.c1 = s.c1;
    p.c2 = mode == 2 ? n.f1 : s.c2;
    p.c3 = mode == 2 ? n.f2 : s.c3;
}
// the head of stn (mode 0: the (3, 3) input transform T) or fstn (mode 1: the (64, 64) feature transform F); mat_user: the
// caller's copy of the matrix, or NULL
inline HeadArgs stn_head(const Net &n, int mode, const float *tmax, int ntiles, float *T, float *F, float *mat_user) {
    const Stn &s = mode == 0 ? n.stn : n.fstn;
    const int K = mode == 0 ? 3 : 64;
    HeadArgs h{};
    h.tmax = tmax; h.ntiles = ntiles;
    h.d1 = s.d1; h.d2 = s.d2; h.d3 = s.d3; h.bn2 = s.bn;
    h.n3 = K * K; h.K = K; h.mat = mode == 0 ? T : F; h.mat_user = mat_user;
    return h;
}
// the classifier's head: feat's dense layers, cls, softmax
inline HeadArgs feat_head(const Net &n, int nc, const float *tmax, int ntiles, float *pooled, float *logits, float *probs) {
    HeadArgs h{};
    h.tmax = tmax; h.ntiles = ntiles;
    h.d1 = n.fd1; h.bn1 = n.fbn1; h.d2 = n.fd2; h.bn2 = n.fbn2; h.d3 = n.cls;
    h.n3 = nc; h.K = 1; h.pooled = pooled; h.logits = logits; h.probs = probs;
    return h;
}

// pointnet_points_kernel<mode> (win: the instantiation that also writes a.tfirst and a.tpre) and pointnet_head_kernel<feat>
// on st; pointnet.hip
fx3d_status launch_points(int mode, bool win, const PointArgs &a, int B, hipStream_t st);
fx3d_status launch_head(bool feat, const HeadArgs &a, int B, hipStream_t st);

__device__ __forceinline__ float bn_sd(const Bn &bn, int o) { return sqrtf(bn.v[o] + kBnEps); }
// what the last layer's BatchNorm is given: relu(acc + bias) for kReluBn, acc + bias for kBnOnly
template <int EPI>
__device__ __forceinline__ float before_bn(float acc, float bias) { return EPI == kReluBn ? relu(acc + bias) : acc + bias; }

// ---- the tile loads: rows beyond the cloud's last point are zeros (they are computed and take part in nothing) ---------------
// the tile of x (3, N, B) as xs[p][3]
__device__ __forceinline__ void load_xs(float *xs, const float *x, int b, int N, int p0, int nvalid) {
    const float *xb = x + ((size_t)b * N + p0) * 3;
    for (int i = threadIdx.x; i < kTile * 3; i += kPtThreads) xs[i] = i < nvalid * 3 ? xb[i] : 0.0f;
}
// the tile of a (64, N, B) array into columns 0 .. 63 of an image
__device__ __forceinline__ void load_tile64(float *img, const float *src, int b, int N, int p0, int nvalid) {
    const float *sb = src + ((size_t)b * N + p0) * 64;
    for (int i = threadIdx.x; i < kTile * 64; i += kPtThreads) img[(i >> 6) * kLd + (i & 63)] = i < nvalid * 64 ? sb[i] : 0.0f;
}

// ---- conv_mfma's walk over the slabs of 32 output channels, with the epilogue left to the caller -----------------------------
// body(o, h, acc0, acc1) while the slab of `in` (row stride LD) times W (CIN, cout) is in the accumulators: o is the lane's
// channel, acc0 / acc1 its 16 points mfma_row(r, h) of the tile's two 32-point halves.  All 4 waves call it.
// CIN = 0: the width is `cin`, known at run time only (MODE 3's first layer): mfma_slab_rt on both halves, so cin needs no padding
// and is never padded (mlp_common.h); W is then read 4-byte aligned (W4: W + cin o is 16-byte aligned for no odd cin).
template <int CIN, int LD = kLd, class Body>
__device__ __forceinline__ void for_each_slab(const float *in, const float *__restrict__ W, int cout, Body body, int cin = CIN) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, j = lane & 31;
    const float *a0 = in + j * LD + h, *a1 = a0 + 32 * LD;
    for (int sl = wave; sl < cout / 32; sl += kPtThreads / 64) {
        const int o = sl * 32 + j;
        if constexpr (CIN == 0) {
            f32x16 acc[2] = {{0}, {0}};
            mfma_slab_rt<LD, 2>(in, W + (size_t)cin * o, cin, h, j, acc);
            body(o, h, acc[0], acc[1]);
        } else {
            f32x16 acc0 = {0}, acc1 = {0};
            mfma_slab<CIN>(a0, a1, W + (size_t)CIN * o, h, acc0, acc1);
            body(o, h, acc0, acc1);
        }
    }
}

// conv_mfma<cin, EPI, false> for a width known at run time only (for_each_slab<0>): out[p][o] = epilogue(sum_c in[p][c] W[c + cin o]),
// o < cout (a multiple of 32); `in` and `out` are two images
template <int EPI, int LD = kLd>
__device__ __forceinline__ void conv_first_rt(const float *in, float *out, int cin, int cout, const Conv &c) {
    for_each_slab<0, LD>(in, c.W, cout, [&](int o, int h, const f32x16 &acc0, const f32x16 &acc1) {
        const float bi = c.b[o], g = c.bn.g[o], be = c.bn.b[o], mu = c.bn.m[o], sd = bn_sd(c.bn, o);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int p = mfma_row(r, h);
            out[p * LD + o] = epilogue<EPI>(acc0[r], bi, g, be, mu, sd);
            out[(p + 32) * LD + o] = epilogue<EPI>(acc1[r], bi, g, be, mu, sd);
        }
    }, cin);
}

// conv_mfma<128, EPI, true> -- the same slabs, epilogue and fold, so the same tmax -- that also finds, while the slab's values
// are still in the accumulators, the first of the tile's valid points whose value EQUALS the tile's maximum (Float32 ==, so
// -0 equals +0; a NaN maximum equals nothing: kNoPoint), and keeps what the BatchNorm was given there.  p0: the tile's first
// point.  A lane's rows mfma_row(r, h) ascend with r, the second half's follow the first's.
template <int EPI>
__device__ __forceinline__ void conv_final_win(const float *in, const Conv &c, int nvalid, int p0, float *__restrict__ tmax,
                                               int32_t *__restrict__ tfirst, float *__restrict__ tpre) {
    for_each_slab<128>(in, c.W, kFeat, [&](int o, int h, const f32x16 &acc0, const f32x16 &acc1) {
        const float bi = c.b[o], g = c.bn.g[o], be = c.bn.b[o], mu = c.bn.m[o], sd = bn_sd(c.bn, o);
        float m = __int_as_float(0xff800000);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int p = mfma_row(r, h);
            if (p < nvalid) m = jmax(m, epilogue<EPI>(acc0[r], bi, g, be, mu, sd));
            if (p + 32 < nvalid) m = jmax(m, epilogue<EPI>(acc1[r], bi, g, be, mu, sd));
        }
        m = jmax(m, __shfl_xor(m, 32, 64));
        int first = kNoPoint;
        float pre = 0.0f;
#pragma unroll
        for (int r = 15; r >= 0; --r) {  // descending, the second half first: the last assignment is the smallest point
            const int p = mfma_row(r, h) + 32;
            if (p < nvalid && epilogue<EPI>(acc1[r], bi, g, be, mu, sd) == m) { first = p0 + p; pre = before_bn<EPI>(acc1[r], bi); }
        }
#pragma unroll
        for (int r = 15; r >= 0; --r) {
            const int p = mfma_row(r, h);
            if (p < nvalid && epilogue<EPI>(acc0[r], bi, g, be, mu, sd) == m) { first = p0 + p; pre = before_bn<EPI>(acc0[r], bi); }
        }
        const int ofirst = __shfl_xor(first, 32, 64);
        const float opre = __shfl_xor(pre, 32, 64);
        if (h == 0) {
            tmax[o] = m;
            tfirst[o] = min(first, ofirst);
            tpre[o] = ofirst < first ? opre : pre;
        }
    });
}

// ---- a round's layers, once ---------------------------------------------------------------------------------------------------
// One block = 64 points of cloud b from p0 on, 4 waves, lds of kPtLds bytes: the tile load, then the round's layers in order,
// each into the image the next reads.  The BatchNorm layers of a round count from 0 (MODE 0, stn: conv1, conv2, conv3; MODE 1,
// fstn: conv_block1, conv1, conv2, conv3; MODE 2, feat: conv1, conv2; MODE 3, stnKD(K) for a.K known at run time only
// (stnkd.hip): MODE 0's layers on x (K, N, B), the tile in columns 0 .. K - 1 of an image and conv1 on mfma_slab_rt, handed to
// the tail as a Layer with CIN = 0); layer STOP is not computed here but handed to
// tail(in, conv, Layer<CIN, COUT, EPI>{}): its input image, its parameters and its shape.  STOP = kLastLayer[MODE] with the
// fold over the tile as the tail is the forward's pointnet_points_kernel; a smaller STOP with the statistics epilogue is
// pointnet_stats_kernel, so the layers below a BatchNorm are the same calls in both.  KEEP_H: MODE 1 stores conv_block1's
// output to a.h.
template <int CIN_, int COUT_, int EPI_>
struct Layer { static constexpr int CIN = CIN_, COUT = COUT_, EPI = EPI_; };
constexpr int kLastLayer[4] = {2, 3, 1, 2};

template <int MODE, int STOP, bool KEEP_H, class Tail>
__device__ __forceinline__ void round_trunk(const PointArgs &a, float *lds, int b, int p0, int nvalid, Tail tail) {
    float *bufA = lds, *bufB = lds + kTile * kLd, *xs = bufB + kTile * kLd, *xt = xs + kTile * 3;
    const int tid = threadIdx.x;
    if constexpr (MODE == 3) gather_centre(bufA, kLd, a.x + (size_t)b * a.N * a.K, a.K, p0, nvalid);
    else if (MODE != 2) load_xs(xs, a.x, b, a.N, p0, nvalid);
    else load_tile64(bufA, a.h, b, a.N, p0, nvalid);
    __syncthreads();
    if constexpr (MODE == 0) {
        if constexpr (STOP == 0) return tail(xs, a.c1, Layer<3, 64, kReluBn>{});
        conv3<kReluBn>(xs, bufA, kLd, 64, a.c1.W, a.c1.b, a.c1.bn);
        __syncthreads();
        if constexpr (STOP == 1) return tail(bufA, a.c2, Layer<64, 128, kReluBn>{});
        conv_mfma<64, kReluBn, false>(bufA, bufB, 128, a.c2.W, a.c2.b, a.c2.bn, nvalid, nullptr);
        __syncthreads();
        tail(bufB, a.c3, Layer<128, kFeat, kReluBn>{});
    } else if constexpr (MODE == 1) {
        conv3<kNone>(xs, xt, 3, 3, a.tf + (size_t)b * 9, nullptr, Bn{});
        __syncthreads();
        if constexpr (STOP == 0) return tail(xt, a.c0, Layer<3, 64, kBnRelu>{});
        conv3<kBnRelu>(xt, bufA, kLd, 64, a.c0.W, a.c0.b, a.c0.bn);
        __syncthreads();
        if constexpr (STOP == 1) return tail(bufA, a.c1, Layer<64, 64, kReluBn>{});
        if (KEEP_H) {
            float *hb = a.h + ((size_t)b * a.N + p0) * 64;
            for (int i = tid; i < nvalid * 64; i += kPtThreads) hb[i] = bufA[(i >> 6) * kLd + (i & 63)];
        }
        conv_mfma<64, kReluBn, false>(bufA, bufB, 64, a.c1.W, a.c1.b, a.c1.bn, nvalid, nullptr);
        __syncthreads();
        if constexpr (STOP == 2) return tail(bufB, a.c2, Layer<64, 128, kReluBn>{});
        conv_mfma<64, kReluBn, false>(bufB, bufA, 128, a.c2.W, a.c2.b, a.c2.bn, nvalid, nullptr);
        __syncthreads();
        tail(bufA, a.c3, Layer<128, kFeat, kReluBn>{});
    } else if constexpr (MODE == 3) {
        if constexpr (STOP == 0) return tail(bufA, a.c1, Layer<0, 64, kReluBn>{});
        conv_first_rt<kReluBn>(bufA, bufB, a.K, 64, a.c1);
        __syncthreads();
        if constexpr (STOP == 1) return tail(bufB, a.c2, Layer<64, 128, kReluBn>{});
        conv_mfma<64, kReluBn, false>(bufB, bufA, 128, a.c2.W, a.c2.b, a.c2.bn, nvalid, nullptr);
        __syncthreads();
        tail(bufA, a.c3, Layer<128, kFeat, kReluBn>{});
    } else {
        conv_mfma<64, kNone, false>(bufA, bufB, 64, a.tf + (size_t)b * 4096, nullptr, Bn{}, nvalid, nullptr);
        __syncthreads();
        if constexpr (STOP == 0) return tail(bufB, a.c2, Layer<64, 128, kReluBn>{});
        conv_mfma<64, kReluBn, false>(bufB, bufA, 128, a.c2.W, a.c2.b, a.c2.bn, nvalid, nullptr);
        __syncthreads();
        tail(bufA, a.c3, Layer<128, kFeat, kBnOnly>{});
    }
}

// ---- the head, phase by phase: one block of kHeadThreads per cloud b, thread tid = one element of each vector -------------------
// Every dense layer is dense_chain over its input in LDS (ascending, from +0.0f).  pointnet_head_kernel is all phases in
// one block; the training-mode heads (pointnet_train.hip) cut them at the BatchNorms; the adjoint's head (pointnet_grad.hip)
// runs the dense phases again and keeps the relus' outputs (its pool also finds the winners).
// MaxPool over the cloud's points into v0 (kFeat), with the classifier's optional copy
template <bool FEAT>
__device__ __forceinline__ void head_pool(const HeadArgs &a, int b, float *v0) {
    const float m = fold_tile_maxima(a.tmax, a.ntiles, b);
    v0[threadIdx.x] = m;
    if (FEAT && a.pooled) a.pooled[(size_t)b * kFeat + threadIdx.x] = m;
}
// relu(dense1): in = v0 (kFeat), NOUT = 512; relu(dense2): in = v1 (512), NOUT = 256; this thread's output, tid < NOUT
template <int NOUT>
__device__ __forceinline__ float head_relu_dense(const Dense &d, const float *in) {
    return relu(dense_chain(in, 2 * NOUT, d.W, NOUT, threadIdx.x) + d.b[threadIdx.x]);
}
// dense3 of v2 (256), output o < n3
__device__ __forceinline__ float head_dense3(const Dense &d, const float *v2, int n3, int o) {
    return dense_chain(v2, 256, d.W, n3, o) + d.b[o];
}
// a head's BatchNorm of this thread's element
__device__ __forceinline__ float head_bn(const Bn &bn, float v) {
    const int tid = threadIdx.x;
    return batchnorm(v, bn.g[tid], bn.b[tid], bn.m[tid], bn_sd(bn, tid));
}
// dense3 of v2 as the transposed (K, K) matrix (T[i,j] = d[j + K i] at i + K j) with the caller's optional copy, or cls, relu
// and the softmax
template <bool FEAT>
__device__ __forceinline__ void head_finish(const HeadArgs &a, int b, const float *v2) {
    for (int o = threadIdx.x; o < a.n3; o += kHeadThreads) {
        const float v = head_dense3(a.d3, v2, a.n3, o);
        if (FEAT) {
            a.logits[(size_t)b * a.n3 + o] = relu(v);
        } else {
            const size_t at = (size_t)b * a.n3 + (o / a.K) + (size_t)a.K * (o % a.K);
            a.mat[at] = v;
            if (a.mat_user) a.mat_user[at] = v;
        }
    }
    if (FEAT) softmax_of_logits(a.logits + (size_t)b * a.n3, a.probs + (size_t)b * a.n3, a.n3);
}

// ---- the fold of a convolution BatchNorm's Float64 tile sums (pointnet_train.hip's and the DGCNN / EdgeConv training-mode
// forward's statistics, pointnet_grad_train.hip's dbeta / dgamma)
constexpr int kFinishGroups = FX3D_POINTNET_STAT_GROUPS;  // interleaved partial sums over (tile, cloud), the header's order
constexpr int kFinishChannels = 16;                       // channels of one finishing block: 256 contiguous bytes per read
constexpr int kFinishThreads = kFinishGroups * kFinishChannels;
// Folds sums (2, C, T) over the T = ntiles B tile sums t = tile + ntiles b of a layer: kFinishGroups chains, chain g over
// t = g, g + kFinishGroups, ... ascending from +0.0, then the chains in ascending g from +0.0; finish(c, s1, s2) in the thread
// that owns channel c.  One block of kFinishThreads = 16 channels; the threads of the last block beyond channel C - 1 (an
// EdgeConv width that is no multiple of 16) read nothing and finish nothing.
template <class Finish>
__device__ __forceinline__ void fold_tile_sums(const double *__restrict__ sums, int C, long long T, Finish finish) {
    __shared__ double p1[kFinishGroups][kFinishChannels], p2[kFinishGroups][kFinishChannels];
    const int cl = threadIdx.x % kFinishChannels, g = threadIdx.x / kFinishChannels;
    const int c = blockIdx.x * kFinishChannels + cl;
    double s1 = 0.0, s2 = 0.0;
    if (c < C)
        for (long long t = g; t < T; t += kFinishGroups) {
            const double *at = sums + 2 * ((size_t)t * C + c);
            s1 = s1 + at[0];
            s2 = s2 + at[1];
        }
    p1[g][cl] = s1;
    p2[g][cl] = s2;
    __syncthreads();
    if (g != 0 || c >= C) return;
    s1 = 0.0; s2 = 0.0;
    for (int k = 0; k < kFinishGroups; ++k) {
        s1 = s1 + p1[k][cl];
        s2 = s2 + p2[k][cl];
    }
    finish(c, s1, s2);
}

// ---- a BatchNorm's batch statistics (pointnet_train.hip; dgcnn_train.hip and edgeconv_train.hip for DGCNN and EdgeConv) ---------
// one BatchNorm's statistics: where they go, and the running values they update
struct StatOut {
    const float *run_m, *run_v;  // the running mean and variance in the parameter buffer
    float *mu, *var;             // the batch statistics buffer
    float *new_m, *new_v;        // the updated running statistics, or NULL
    float mtm;
    long long m;                 // values per channel: N B after a convolution (K N B in an EdgeConv), B after a dense layer
};

// the header's "mean and variance" and "running statistics", for channel c with the sums S1, S2 over its m values
__device__ __forceinline__ void finish_channel(const StatOut &o, int c, double S1, double S2) {
    const double dm = (double)o.m;
    const double mu64 = S1 / dm;
    double v64 = S2 / dm - mu64 * mu64;
    v64 = v64 < 0.0 ? 0.0 : v64;  // (a NaN stays)
    const float mu = (float)mu64, var = (float)v64;
    o.mu[c] = mu;
    o.var[c] = var;
    if (o.new_m) {
        const float keep = 1.0f - o.mtm;
        o.new_m[c] = (keep * o.run_m[c]) + (o.mtm * mu);
        o.new_v[c] = (keep * o.run_v[c]) + (((o.mtm * (float)o.m) / (float)(o.m - 1)) * var);
    }
}

// a tile's sums of one channel: the rows p of the tile with bit 2 of p equal to h are one chain in ascending p (what a lane
// of half-wave h holds of a slab, mfma_row), and the tile's sum is chain(0) + chain(1).  (An EdgeConv's chains are per 32-point
// half and run over the neighbour rank as well: edgeconv_train.hip.)
struct TileSum {
    double s1 = 0.0, s2 = 0.0;
    __device__ __forceinline__ void add(float v) {
        const double d = (double)v;
        s1 = s1 + d;
        s2 = s2 + d * d;  // the product of two Float32 is exact in Float64
    }
};
// TileSum for (gy, gy xh), the sums of a training-mode adjoint's dbeta and dgamma (pointnet_grad_train.hip, edgeconv_grad_train.hip)
struct PairSum {
    double s1 = 0.0, s2 = 0.0;
    __device__ __forceinline__ void add(float gy, float xh) {
        const double d = (double)gy;
        s1 = s1 + d;
        s2 = s2 + d * (double)xh;  // the product of two Float32 is exact in Float64
    }
};
__device__ __forceinline__ void store_tile_sum(double *sums, int o, double s1, double s2) {
    sums[2 * o] = s1;
    sums[2 * o + 1] = s2;
}

// a convolution on the MFMA whose BatchNorm's statistics are wanted: conv_mfma's slabs (for_each_slab) with the statistics
// epilogue.  sums: the tile's (2, cout).  CIN = 0: the width is `cin` (for_each_slab).
template <int CIN, int EPI, int LD = kLd>
__device__ __forceinline__ void conv_stat_mfma(const float *in, int cout, const float *__restrict__ W, const float *__restrict__ bias,
                                               int nvalid, double *__restrict__ sums, int cin = CIN) {
    for_each_slab<CIN, LD>(in, W, cout, [&](int o, int h, const f32x16 &acc0, const f32x16 &acc1) {
        const float bi = bias[o];
        TileSum t;
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (mfma_row(r, h) < nvalid) t.add(before_bn<EPI>(acc0[r], bi));
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (mfma_row(r, h) + 32 < nvalid) t.add(before_bn<EPI>(acc1[r], bi));
        const double o1 = __shfl_xor(t.s1, 32, 64), o2 = __shfl_xor(t.s2, 32, 64);
        if (h == 0) store_tile_sum(sums, o, t.s1 + o1, t.s2 + o2);
    }, cin);
}

// pointnet_train.hip's two finishing kernels on st.  launch_stat_finish: the fold of a layer's tile sums (2, C, T), T = ntiles B,
// then mean, variance and running statistics of its C channels.  launch_dense_stats: a dense BatchNorm, thread c sums channel c
// of act (C, B), C a multiple of 256, over the clouds in ascending b from +0.0 and finishes it.  label: the launch's name in the
// library's profile.
fx3d_status launch_stat_finish(const double *sums, int C, long long T, const StatOut &o, hipStream_t st, const char *label);
fx3d_status launch_dense_stats(const float *act, int C, int B, const StatOut &o, hipStream_t st, const char *label);

// pointnet_train.hip's statistics pass and its heads cut at their BatchNorms, for stnkd.hip as well
struct StatArgs {
    PointArgs p;
    double *sums;  // (2, C, ntiles, B) for the C channels of the layer
};
struct TrainHeadArgs {
    HeadArgs h;            // the test-mode head's arguments, bn1 / bn2 at the batch statistics
    float *a1, *a2;        // workspace: relu(dense1) (512, B), FEAT only; relu(dense2) [times the dropout multiplier] (256, B)
    const float *dropout;  // FEAT: (256, B) multipliers or NULL
};
// pointnet_stats_kernel<mode, L> on st: the tile sums of BatchNorm L of round `mode` (round_trunk's modes, 3 = stnKD(K))
fx3d_status launch_stats(int mode, int L, const StatArgs &s, int B, hipStream_t st);
// part 0 = head_a (MaxPool, relu(dense1); stn / fstn: relu(dense2) too), 1 = head_b (feat), 2 = head_c (BatchNorm(256), the end)
fx3d_status launch_train_head(int part, bool feat, const TrainHeadArgs &t, int B, hipStream_t st);

// ---- what the two adjoints (pointnet_grad.hip, pointnet_grad_train.hip) share ------------------------------------------------------
// the gradient's block of a conv layer with its BatchNorm: W | b | gamma | beta | mu | var
struct GradBlock { float *W, *b, *g, *be, *m, *v; };

// a segment of a tile partial and where its chain over the partials goes ("PointNet adjoint": b ascending, tile ascending)
struct Seg { int at; float *dst; int n, nz; };
constexpr int kMaxSegs = 3;
struct ReduceArgs { const float *part; Seg s[kMaxSegs]; int psize, nparts; };
inline float *mut(const float *p) { return const_cast<float *>(p); }
inline GradBlock grad_block(const Conv &c) { return GradBlock{mut(c.W), mut(c.b), mut(c.bn.g), mut(c.bn.b), mut(c.bn.m), mut(c.bn.v)}; }
inline GradBlock grad_block(const Bn &bn) { return GradBlock{nullptr, nullptr, mut(bn.g), mut(bn.b), mut(bn.m), mut(bn.v)}; }

// pointnet_grad.hip's finishing kernels on st: the chains over `nparts` partials of `psize` floats for the nsegs segments of ra;
// the same per cloud (dst[e + n b] over the cloud's ntiles partials); a dense layer's sums over the clouds
fx3d_status launch_reduce(const ReduceArgs &ra, int nsegs, hipStream_t st);
fx3d_status launch_cloud_reduce(const float *part, int psize, int at, int ntiles, int n, int B, float *dst, hipStream_t st);
fx3d_status launch_dense_sums(const DenseSums &q, hipStream_t st);

// out[c + cin o] = the chain from +0 over the tile's 64 rows, ascending, of fmaf(A[p][c], D[p][o], acc); cin and cout multiples
// of 32.  v_mfma_f32_32x32x2_f32 takes two rows per instruction, the lower first: lane (h, j) gives A[p + h][c0 + j] and
// D[p + h][o0 + j], and holds the result's rows c0 + mfma_row(r, h) of column o0 + j.  Rows beyond the cloud have D = +0.
__device__ __forceinline__ void hsum_mfma(const float *A, const float *D, int cin, int cout, float *__restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, j = lane & 31;
    const int nci = cin / 32, nt = nci * (cout / 32);
    for (int t = wave; t < nt; t += kPtThreads / 64) {
        const int c0 = (t % nci) * 32, o0 = (t / nci) * 32;
        const float *ap = A + h * kLd + c0 + j, *dp = D + h * kLd + o0 + j;
        f32x16 acc = {0};
#pragma unroll 8
        for (int p = 0; p < kTile; p += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[p * kLd], dp[p * kLd], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) out[c0 + mfma_row(r, h) + (size_t)cin * (o0 + j)] = acc[r];
    }
}

// out[p][c] = the chain from +0 over o < COUT, ascending, of fmaf(dz[p][o], W[c + cin o], acc) for the tile's 64 rows and
// c < cin (a multiple of 32), W as the forward reads it.  A wave owns (32 channels) x (one 32-point half) at a time.
template <int COUT>
__device__ __forceinline__ void back_mfma(const float *dz, float *out, int cin, const float *__restrict__ W) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, j = lane & 31;
    for (int t = wave; t < 2 * (cin / 32); t += kPtThreads / 64) {
        const int half = t & 1, c = (t >> 1) * 32 + j;
        const float *ap = dz + (half * 32 + j) * kLd + h, *wp = W + c + (size_t)cin * h;
        f32x16 acc = {0};
#pragma unroll 8
        for (int o = 0; o < COUT; o += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[o], wp[(size_t)cin * o], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) out[(half * 32 + mfma_row(r, h)) * kLd + c] = acc[r];
    }
}

// H[c + 3 o] = the chain over the tile's valid rows of fmaf(xs[p][c], d[p][o], acc), c < 3, o < 64: threads first .. first + 191
__device__ __forceinline__ void hsum3(const float *xs, const float *d, int nvalid, int first, float *__restrict__ out) {
    const int e = threadIdx.x - first;
    if (e < 0 || e >= 192) return;
    const int o = e / 3, c = e - 3 * o;
    float acc = 0.0f;
    for (int p = 0; p < nvalid; ++p) acc = fmaf(xs[p * 3 + c], d[p * kLd + o], acc);
    out[e] = acc;
}

// ---- what the training-mode adjoints (pointnet_grad_train.hip, dgcnn_grad_train.hip) share ------------------------------------------
// the header's "gradient at the BatchNorm's input": every operation rounded, nothing fused (-ffp-contract=off)
__device__ __forceinline__ float bn_gv(float gy, float xh, float mb, float mg, float gam, float sd) {
    float t = gy - mb;
    t = t - (xh * mg);
    return (t * gam) / sd;
}

// one BatchNorm's sums: where dgamma, dbeta and the +0 of mu / var go, and the two means the layer below needs
struct BnOut {
    GradBlock g;
    float *mb, *mg;  // (C) each: Float32(dbeta64 / m), Float32(dgamma64 / m)
    long long m;
};
__device__ __forceinline__ void finish_bn(const BnOut &o, int c, double s1, double s2) {
    const double dm = (double)o.m;
    o.g.be[c] = (float)s1;
    o.g.g[c] = (float)s2;
    o.g.m[c] = 0.0f;
    o.g.v[c] = 0.0f;
    o.mb[c] = (float)(s1 / dm);
    o.mg[c] = (float)(s2 / dm);
}

// pointnet_grad_train.hip's pointnet_gt_cloud_sums_kernel on st: a BatchNorm whose values are (C, B), C a multiple of 256: thread c,
// one Float64 chain over b ascending; with nstar (C, B) over the clouds that have a winner (nstar >= 0)
fx3d_status launch_cloud_sums(const float *gy, const float *xh, const int32_t *nstar, int C, int B, const BnOut &o, hipStream_t st);

// A lane's channel o of a maximum's last convolution (1024 outputs), cloud b, tile from point p0: its constants, and d of a point
// from the accumulator's value.  a: the kernel's arguments with nstar, gy3 (1024, B) and mb, mg (1024).  EPI: kReluBn / kBnOnly
// (PointNet's rounds: relu below the BatchNorm masks d) or kBnRelu (DGCNN's conv_3: the relu is above the BatchNorm and already
// in gy3, what the BatchNorm is given is conv + bias).
template <int EPI>
struct LastChannel {
    float bi, gam, mu, sd, mb, mg, gy;
    int win;  // the winner's row in this tile (any other value: not in this tile)
    template <class Args>
    __device__ __forceinline__ LastChannel(const Conv &c, const Args &a, int o, int b, int p0) {
        bi = c.b[o]; gam = c.bn.g[o]; mu = c.bn.m[o]; sd = bn_sd(c.bn, o); mb = a.mb[o]; mg = a.mg[o];
        gy = a.gy3[(size_t)b * kFeat + o];
        const int n = a.nstar[(size_t)b * kFeat + o];
        win = n < 0 ? -1 : n - p0;
    }
    __device__ __forceinline__ float d(float acc, int p) const {
        const float pre = before_bn<EPI>(acc, bi);
        const float g = bn_gv(p == win ? gy : 0.0f, (pre - mu) / sd, mb, mg, gam, sd);
        return (EPI == kReluBn && !(pre > 0.0f)) ? 0.0f : g;
    }
    // the slab's d of the tile's valid rows (+0 beyond them) into column `col` of the image D (row stride kLd)
    __device__ __forceinline__ void store(float *D, int col, int h, int nvalid, const f32x16 &acc0, const f32x16 &acc1) const {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int p = mfma_row(r, h);
            D[p * kLd + col] = p < nvalid ? d(acc0[r], p) : 0.0f;
            D[(p + 32) * kLd + col] = p + 32 < nvalid ? d(acc1[r], p + 32) : 0.0f;
        }
    }
};

// ---- the dense adjoint of a maximum's last convolution (CIN -> 1024): PointNet's three rounds (CIN = 128, the image stride kLd) and
// DGCNN's conv_3 (CIN = 256, kLd3).  pointnet_gt_last_{bwd,pgrad}_kernel and dgcnn_gt_conv3_{bwd,pgrad}_kernel are these two bodies.
constexpr int kGroup = 128;         // the last layer's outputs per step: one slab per wave of a tile kernel
constexpr int kPgradThreads = 512;  // last_pgrad: 8 waves, two per slab of the group
static_assert(kGroup == 32 * (kPtThreads / 64), "one slab per wave");

struct LastArgs {
    const float *in;       // (CIN, N, B): the last convolution's input (last_pgrad; DGCNN's last_back)
    Conv c3;               // the last convolution, at the batch statistics
    const int32_t *nstar;  // (1024, B)
    const float *gy3;      // (1024, B): the gradient at the last BatchNorm's output, at the winner
    const float *mb, *mg;  // (1024)
    float *g;              // (CIN, N, B): the gradient at the last convolution's input
    float *Hc, *hc;        // (CIN, 1024, B), (1024, B): dW and db of each cloud
    int N, ntiles;
};

// The way back, one block = the 64 points of cloud b from p0 on, whose rows of the input are the image `in` (row stride LD): the
// slabs (for_each_slab) four at a time -- kGroup outputs, one slab per wave --; while a slab is in the accumulators LastChannel
// forms the gradient at the contraction and writes it to the image D (row stride kLd); all four waves then carry the chain over
// those 128 outputs on v_mfma_f32_32x32x2_f32 (back_mfma's operands) into the tiles t = wave + 4 u of (CIN / 32 input channels) x
// (2 halves), as back_mfma numbers them, CIN / 64 per wave, kept across the eight groups: one chain over all 1024 outputs
// ascending.  Stores a.g.
template <int CIN, int LD, int EPI>
__device__ __forceinline__ void last_back(const float *in, float *D, const Conv &c, const LastArgs &a, int b, int p0, int nvalid) {
    constexpr int NU = CIN / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, j = lane & 31;
    f32x16 back[NU] = {};
    for_each_slab<CIN, LD>(in, c.W, kFeat, [&](int o, int, const f32x16 &acc0, const f32x16 &acc1) {
        const int col = o & (kGroup - 1), o0 = o - col;  // every wave is in the same group of 128 outputs
        LastChannel<EPI>(c, a, o, b, p0).store(D, col, h, nvalid, acc0, acc1);
        __syncthreads();
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int t = wave + 4 * u, half = t & 1, ci = (t >> 1) * 32 + j;
            const float *ap = D + (half * 32 + j) * kLd + h, *wp = c.W + ci + (size_t)CIN * (o0 + h);
#pragma unroll 8
            for (int q = 0; q < kGroup; q += 2)
                back[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[q], wp[(size_t)CIN * q], back[u], 0, 0, 0);
        }
        __syncthreads();
    });
    float *g = a.g + ((size_t)b * a.N + p0) * CIN;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int t = wave + 4 * u, half = t & 1, ci = (t >> 1) * 32 + j;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int p = half * 32 + mfma_row(r, h);
            if (p < nvalid) g[(size_t)p * CIN + ci] = back[u][r];
        }
    }
}

// Block (k, b) of kPgradThreads: dW[i, o] and db[o] of cloud b for o in [128 k, 128 k + 128): one chain over the cloud's points
// ascending.  lds: the image of a tile of a.in (row stride LD), then D (kLd).  8 waves: wave w recomputes slab w & 3 of the group for
// the 32-point half w >> 2 (mfma_slab_rt on one half: the forward's chain), forms d again (LastChannel) and owns the CIN / 64
// (32 x 32) tiles of dW with the input channels (CIN / 2) (w >> 2) .. + CIN / 2 - 1 and the outputs of slab w & 3 (hsum_mfma's
// operands); db is one Float32 chain per output.
template <int CIN, int LD, int EPI>
__device__ __forceinline__ void last_pgrad(float *lds, const LastArgs &a) {
    constexpr int NU = CIN / 64, kUnroll = 16 / NU;  // 16 MFMAs in the unrolled body
    float *A = lds, *D = lds + kTile * LD;
    const int b = blockIdx.y, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6, h = lane >> 5, j = lane & 31, part = wave >> 2;
    const int o0 = blockIdx.x * kGroup, col = (wave & 3) * 32 + j, o = o0 + col;
    f32x16 H[NU] = {};  // rows (CIN / 2) part + 32 u + mfma_row(r, h) of column o
    float sb = 0.0f;
    for (int tile = 0; tile < a.ntiles; ++tile) {
        const int p0 = tile * kTile;
        const int nvalid = min(kTile, a.N - p0);
        const float *src = a.in + ((size_t)b * a.N + p0) * CIN;
        for (int i = tid; i < kTile * CIN; i += kPgradThreads) A[((unsigned)i / CIN) * LD + ((unsigned)i % CIN)] = i < nvalid * CIN ? src[i] : 0.0f;
        __syncthreads();
        {
            f32x16 acc[1] = {{0}};
            mfma_slab_rt<LD, 1>(A + part * 32 * LD, a.c3.W + (size_t)CIN * o, CIN, h, j, acc);
            const LastChannel<EPI> ch(a.c3, a, o, b, p0);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int p = part * 32 + mfma_row(r, h);
                D[p * kLd + col] = p < nvalid ? ch.d(acc[0][r], p) : 0.0f;
            }
        }
        __syncthreads();
        if (tid < kGroup)
            for (int p = 0; p < nvalid; ++p) sb = sb + D[p * kLd + tid];
        const float *dp = D + h * kLd + col, *ap = A + h * LD + (CIN / 2) * part + j;
#pragma unroll kUnroll
        for (int p = 0; p < kTile; p += 2) {
            const float d = dp[p * kLd];
#pragma unroll
            for (int u = 0; u < NU; ++u) H[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[p * LD + 32 * u], d, H[u], 0, 0, 0);
        }
        __syncthreads();
    }
    float *out = a.Hc + ((size_t)b * kFeat + o) * CIN + (CIN / 2) * part;
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) out[32 * u + mfma_row(r, h)] = H[u][r];
    if (tid < kGroup) a.hc[(size_t)b * kFeat + o0 + tid] = sb;
}

// a kernel with dynamic LDS on a (nx, B) grid, under its label in the library's profile
template <class K, class... A>
inline fx3d_status launch_tile(K kernel, const char *name, const char *label, size_t lds, int nx, int B, int threads, hipStream_t st,
                               const A &...a) {
    const fx3d_status rc = ensure_dynamic_lds(reinterpret_cast<const void *>(kernel), (int)lds, name);
    if (rc != FX3D_OK) return rc;
    ProfileScope prof(label, st);
    hipLaunchKernelGGL(kernel, dim3(nx, B), dim3(threads), lds, st, a...);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

}  // namespace pointnet
}  // namespace mlp
}  // namespace fx3d
