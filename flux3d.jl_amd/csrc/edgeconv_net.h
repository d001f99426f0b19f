// What edgeconv.hip (the forward) and edgeconv_train.hip (the training-mode forward) share: the kernel's arguments, a hidden
// layer from image to image, the loop over the neighbour rank k with its last layer left to the caller (edge_trunk), and on the
// host the LDS plan, the workspace, the neighbour search and the forward kernel's launch.
#pragma once
#include "mlp_common.h"

namespace fx3d {
namespace mlp {

struct EdgeConvArgs {
    const float *x;      // (F, N, B)
    const int32_t *idx;  // (K, N, B), 0-based
    float *out;          // (cL, N, B)
    Conv c[kMaxLayers];
    int w[kMaxLayers + 1];  // F, c1, ..., cL
    int nl, cout;           // L, cL
    int N, K;
    int img0, img1;         // offsets of the two hidden images from `rows` (floats)
    int shared_rows;        // img1 is `rows`: the x_n half is gathered with every k
};

// Who computes what of a layer of `cout` channels.  Beyond 64 channels a wave owns the slabs wave, wave + 4, ... of 32 channels
// for both 32-point halves of the tile (one weight load feeds four MFMAs).  Up to 64 channels there are two slabs at most, and
// two of the four waves would idle: there a wave owns ONE half of one slab -- slab wave / 2, half wave % 2.
__device__ __forceinline__ bool split_halves(int cout) { return cout <= 64; }

// one slab (NH = 2) or one half of it (NH = 1, half `half`) of a hidden layer:
// out[p][o] = relu(BN(sum_c in[p][c] W[c + cin o] + b[o])) for o < cout
template <int LD, int NH>
__device__ __forceinline__ void conv_item(const float *in, float *out, int cin, int cout, const Conv &c, int sl, int half) {
    const int lane = threadIdx.x & 63, h = lane >> 5, j = lane & 31;
    const int o = sl * 32 + j, oc = min(o, cout - 1);  // oc: what a lane beyond a partial slab reads
    f32x16 acc[NH];
#pragma unroll
    for (int t = 0; t < NH; ++t) acc[t] = f32x16{0};
    mfma_slab_rt<LD, NH>(in + half * 32 * LD, c.W + (size_t)cin * oc, cin, h, j, acc);
    const float bi = c.b[oc], g = c.bn.g[oc], be = c.bn.b[oc], mu = c.bn.m[oc], sd = sqrtf(c.bn.v[oc] + kBnEps);
    if (o < cout) {
        float *ob = out + (half * 32) * LD + o;
#pragma unroll
        for (int r = 0; r < 16; ++r)
#pragma unroll
            for (int t = 0; t < NH; ++t) ob[(t * 32 + mfma_row(r, h)) * LD] = epilogue<kBnRelu>(acc[t][r], bi, g, be, mu, sd);
    }
}

// one hidden layer, from image to image, for the tile's 64 points
template <int LD>
__device__ __forceinline__ void conv_rt(const float *in, float *out, int cin, int cout, const Conv &c) {
    const int wave = threadIdx.x >> 6;
    if (split_halves(cout)) {
        if ((wave >> 1) * 32 < cout) conv_item<LD, 1>(in, out, cin, cout, c, wave >> 1, wave & 1);
    } else {
        for (int sl = wave; sl * 32 < cout; sl += kPtThreads / 64) conv_item<LD, 2>(in, out, cin, cout, c, sl, 0);
    }
}

// One block = 64 points of cloud b from p0 on, 4 waves: the loop over the neighbour rank k.  Per k the gather of the edge rows
// and the hidden layers 1 .. L - 1 from image to image; the LAST layer of a.nl is not computed here but handed to
// last(in, cin, cout, conv): its input image, its shape and its parameters.  With the fold into the running maxima as `last`
// this is edgeconv_kernel; with the statistics epilogue, on arguments cut at layer l, it is edgeconv_stats_kernel: the gather
// and the layers below a BatchNorm are the same calls in both.
template <int LD, class Last>
__device__ __forceinline__ void edge_trunk(const EdgeConvArgs &a, float *lds, int b, int p0, int nvalid, Last last) {
    float *rows = lds, *img0 = lds + a.img0, *img1 = lds + a.img1;
    const int F = a.w[0], L = a.nl, cout = a.cout;
    const float *xb = a.x + (size_t)b * a.N * F;
    const int32_t *ib = a.idx + ((size_t)b * a.N + p0) * a.K;
    if (!a.shared_rows) gather_centre(rows, LD, xb, F, p0, nvalid);
    __syncthreads();
    for (int k = 0; k < a.K; ++k) {
        if (a.shared_rows) gather_centre(rows, LD, xb, F, p0, nvalid);  // (gather_diff reads what the same thread wrote)
        gather_diff(rows, LD, xb, ib, F, a.N, a.K, k, p0, nvalid);
        __syncthreads();
        // the layers: one copy of the code, its layer picked by wave-uniform selects among the kernel arguments (a constant
        // index in every access, so that a.c[] and a.w[] stay in scalar registers)
        const float *src = rows;
        float *dst = img0;
        int cin = 2 * F;
        for (int i = 0; i + 1 < L; ++i) {
            const Conv c = i == 0 ? a.c[0] : i == 1 ? a.c[1] : a.c[2];
            const int co = i == 0 ? a.w[1] : i == 1 ? a.w[2] : a.w[3];
            conv_rt<LD>(src, dst, cin, co, c);
            __syncthreads();
            src = dst;
            dst = i == 0 ? img1 : img0;
            cin = co;
        }
        last(src, cin, cout, L == 1 ? a.c[0] : L == 2 ? a.c[1] : L == 3 ? a.c[2] : a.c[3]);
        // The next k's writes.  `rows` was last read by the first layer, before a barrier above -- unless the last layer itself
        // read it (L = 1) or img1, which the last layer of L = 3 read, is `rows`: then the waves meet here first.  img0 / img1 are
        // written again only after the barrier that follows the next gather, which a wave reaches after its last layer.
        if (L == 1 || (L == 3 && a.shared_rows)) __syncthreads();
    }
}

// ---- the host side -------------------------------------------------------------------------------------------------
// the LDS images: one stride for all, from the widest layer input
inline void lds_plan(const int32_t *layers, int nlayers, EdgeConvArgs *a, int *ld, size_t *bytes) {
    int widest = 2 * layers[0];
    for (int i = 1; i + 1 < nlayers; ++i) widest = layers[i] > widest ? layers[i] : widest;
    *ld = edge_stride(widest);
    const int L = nlayers - 1, image = kTile * *ld;
    int nimg = L >= 3 ? 3 : L;
    a->shared_rows = (size_t)nimg * image * sizeof(float) > kMaxLds;
    if (a->shared_rows) nimg = 2;
    a->img0 = L >= 2 ? image : 0;
    a->img1 = L >= 3 && !a->shared_rows ? 2 * image : 0;
    *bytes = (size_t)nimg * image * sizeof(float);
}

// the forward's workspace: the neighbour lists (K, N, B) | the neighbour search's scratch
struct EdgeWsPlan { size_t idx, knn, knn_bytes, total; };
inline fx3d_status edge_ws_plan(int F, int N, int B, int K, EdgeWsPlan *w) {
    WsBump ws;
    w->idx = ws.put((size_t)K * N * B * sizeof(int32_t));
    const fx3d_status rc = fx3d_knn_workspace_bytes(N, N, B, F, K, 1, &w->knn_bytes);
    if (rc != FX3D_OK) return rc;
    w->knn = ws.put(w->knn_bytes);
    w->total = ws.at;
    return FX3D_OK;
}

// The arguments of one pass over the first `nlayers` entries of `layers` (the whole layer, or the layer cut at a BatchNorm whose
// statistics are wanted), with the LDS plan of exactly those layers.  stats: NULL, or the statistics buffer in the layout of
// "DGCNN / EdgeConv training-mode forward" -- per BatchNorm mu (C), then sigma2 (C) -- from which the BatchNorms read their mean
// and variance instead of the running values of the parameter buffer.
struct EdgePass { EdgeConvArgs a; int ld; size_t lds_bytes; };
inline EdgePass edge_pass(const float *params_dev, const float *stats, const int32_t *layers, int nlayers, int K, const float *x, int N,
                          const int32_t *idx, float *out) {
    EdgePass p{};
    EdgeConvArgs &a = p.a;
    edgeconv_layout(params_dev, layers, nlayers, a.c);
    if (stats) {
        size_t at = 0;
        for (int i = 1; i < nlayers; ++i) {
            a.c[i - 1].bn.m = stats + at;
            a.c[i - 1].bn.v = stats + at + layers[i];
            at += 2 * (size_t)layers[i];
        }
    }
    for (int i = 0; i < nlayers; ++i) a.w[i] = layers[i];
    a.nl = nlayers - 1; a.cout = layers[nlayers - 1];
    a.N = N; a.K = K; a.x = x; a.idx = idx; a.out = out;
    lds_plan(layers, nlayers, &a, &p.ld, &p.lds_bytes);
    return p;
}

// edgeconv.hip: the lists the pass uses -- idx_in, or the search's (fx3d_knn_ws on the cloud's own rows, rank 0 dropped) into
// idx_out or, without one, the workspace -- and edgeconv_kernel on st
fx3d_status edgeconv_neighbours(const float *x, int F, int N, int B, int K, const int32_t *idx_in, int32_t *idx_out, void *ws,
                                fx3d_stream_t s, const int32_t **idx);
fx3d_status edgeconv_launch(const EdgePass &p, int B, hipStream_t st, const char *label);


// edgeconv_train.hip: EdgeConv in training mode on x (F, N, B), for fx3d_edgeconv_forward_train and both stages of
// fx3d_dgcnn_forward_train.  The arguments are fx3d_edgeconv_forward_train's (flux3d_hip.h), already checked; ws: the forward's
// workspace (edgeconv_workspace_bytes); sums: edgeconv_train_sums_bytes of scratch for the tile sums, 8-byte aligned; the labels
// name the launches in the library's profile.  edgeconv_stat_count: the floats of the layer's statistics buffer.
struct EdgeTrainLabels { const char *stats, *stats_last, *finish, *closing; };
long long edgeconv_stat_count(const int32_t *layers, int nlayers);
size_t edgeconv_train_sums_bytes(const int32_t *layers, int nlayers, int N, int B);
fx3d_status edgeconv_train_run(const float *params_dev, const int32_t *layers, int nlayers, int K, const float *x, int N, int B,
                               const int32_t *idx_in, float momentum, float *out, int32_t *idx_out, float *batch_stats, float *running,
                               void *ws, double *sums, fx3d_stream_t s, const EdgeTrainLabels &lb);

}  // namespace mlp
}  // namespace fx3d
