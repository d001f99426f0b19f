// What the EdgeConv parameter adjoint (edgeconv_pgrad.hip) and the training-mode adjoint's closing pass (edgeconv_grad_train.hip)
// share: the fused kernel -- edgeconv_pgrad.hip's header comment describes it -- with its contraction (take), the arguments of the
// finishing kernels and the chain over the chunk partials (launch_pgrad_reduce, defined in edgeconv_pgrad.hip), and on the host the
// kernel's plan and the workspace.
#pragma once
#include "edgeconv_adjoint.h"

namespace fx3d {
namespace mlp {

constexpr int kGradChunk = FX3D_EDGECONV_GRAD_CHUNK;
constexpr int kGradTiles = kGradChunk / 32;

struct PgradArgs : AdjointArgs {
    float *part;                             // (psize, chunks, B): the chunk partials
    int woff[kMaxLayers], boff[kMaxLayers];  // W_l and b_l in the parameter buffer (floats)
    int psize;
    unsigned int lmin;                       // 4 bits per pass: the lowest layer that has a tile in it
};

// the tiles of one layer in a wave's list: its slabs (wave, wave + 4, ... below cout) times the layer's input tiles
__device__ __forceinline__ int wave_slabs(int cout, int wave) { return max(0, ((cout + 31) / 32 - wave + kWaves - 1) / kWaves); }

// The wave's slab sl of d_l (this lane: channel sl 32 + j, rows mfma_row(r, h)) against a_{l-1} in `ain` (cin channels): the h
// chain of the slab (hs: one per slab of the wave) and the slab's input tiles.  first: the layer's first tile in the wave's list,
// less the pass's first.
template <int LD, int NT, int NS>
__device__ __forceinline__ void take(f32x16 (&H)[NT], float (&hs)[NS], f32x16 d, int sl, int wave, int nvalid, int first,
                                     const float *ain, int cin, int h, int j) {
#pragma unroll
    for (int r = 0; r < 16; ++r) d[r] = mfma_row(r, h) < nvalid ? d[r] : 0.0f;
    const int s = __builtin_amdgcn_readfirstlane((sl - wave) / kWaves);  // (hidden_bwd's slab index is no scalar to the compiler)
#pragma unroll
    for (int q = 0; q < NS; ++q)
        if (s == q) {
#pragma unroll
            for (int r = 0; r < 16; ++r) hs[q] = hs[q] + d[r];
        }
    // the slab's input tiles are the register tiles t0 .. t0 + nci - 1 where they are this pass's: one static tile after the other
    const int nci = (cin + 31) / 32, t0 = first + s * nci;
    const float *a0 = ain + 4 * h * LD;  // row mfma_row(r, h) is 4 h + mfma_row(r, 0)
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int ci = i - t0;
        if (ci < 0 || ci >= nci) continue;  // wave-uniform
        const float *ap = a0 + min(ci * 32 + j, cin - 1);
#pragma unroll
        for (int r = 0; r < 16; ++r) H[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[mfma_row(r, 0) * LD], d[r], H[i], 0, 0, 0);
    }
}

// the training-mode instantiation's arguments (edgeconv_adjoint.h: TrainBn; stop = 0, nvalid set per tile), and the mode of either
struct PgradTrainArgs : PgradArgs { TrainBn bn; };
__device__ __forceinline__ EvalBn mode_of(const PgradArgs &, int) { return EvalBn{}; }
__device__ __forceinline__ TrainBn mode_of(const PgradTrainArgs &a, int nvalid) {
    TrainBn m = a.bn;
    m.nvalid = nvalid;
    return m;
}

// Args = PgradTrainArgs: the closing pass of the training-mode adjoint.  The same chunk loop, tile lists, take, passes, LDS plan and
// flush; the steps write gv_l where they wrote dz_l, and the sinks contract gv_l (not d_l) with a_{l-1}: H_l is dW_l, h_l is db_l.
template <int LD, int NS, int NT, class Args = PgradArgs>
__global__ __launch_bounds__(kPtThreads) void edgeconv_pgrad_kernel(const Args a) {
    extern __shared__ float lds[];
    constexpr bool kTrain = decltype(mode_of(a, 0))::kTrain;
    constexpr int T = 32, IMG = T * LD;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), h = lane >> 5, j = lane & 31;
    const int b = blockIdx.y, chunk = blockIdx.x, t0 = blockIdx.z * NT;
    const int F = a.w[0], L = a.nl, cout = a.cout;
    const bool sums = a.gx != nullptr && blockIdx.z == 0;  // the input gradient: pass 0
    const int lmin = (a.lmin >> (4 * blockIdx.z)) & 15;    // this pass needs d_l for l >= lmin only: the walk back ends there
    const float *xb = a.x + (size_t)b * a.N * F;
    float *rows = lds;
    float *dzl = L == 1 ? lds + IMG : L == 2 ? lds + 2 * IMG : lds;  // where dz_L goes
    // the last layer by wave-uniform selects among the kernel arguments (a constant index in every access, as edgeconv_kernel)
    const Conv cl = L == 1 ? a.c[0] : L == 2 ? a.c[1] : L == 3 ? a.c[2] : a.c[3];
    const int cinl = L == 1 ? 2 * F : L == 2 ? a.w[1] : L == 3 ? a.w[2] : a.w[3];  // its input width
    // the wave's tile list: base[i] = the first tile of layer i + 1
    int base[kMaxLayers];
    {
        int at = 0;
#pragma unroll
        for (int i = 0; i < kMaxLayers; ++i) {
            base[i] = at;
            if (i < L) at += wave_slabs(a.w[i + 1], wave) * (((i == 0 ? 2 * F : a.w[i]) + 31) / 32);
        }
    }
    const int basel = (L == 1 ? base[0] : L == 2 ? base[1] : L == 3 ? base[2] : base[3]) - t0;

    f32x16 H[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) H[i] = f32x16{0};
    float hl[NS], hh[kMaxLayers - 1][NS];  // the h chains of this half-wave: layer L, and layers 1 .. 3 where they are hidden
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        hl[s] = 0.0f;
#pragma unroll
        for (int i = 0; i < kMaxLayers - 1; ++i) hh[i][s] = 0.0f;
    }

    for (int tile = 0; tile < kGradTiles; ++tile) {
        const int p0 = chunk * kGradChunk + tile * T;
        if (p0 >= a.N) break;  // block-uniform
        const int nvalid = min(T, a.N - p0);
        const int32_t *ib = a.idx + ((size_t)b * a.N + p0) * a.K;
        f32x16 tgt[NS][1], gv[NS][1], S[NS][1];
        float dz0[NS];
        const float nan = quiet_nan();
        // the target load (kept here, not a step of edgeconv_adjoint.h: as one, this kernel spilled to scratch at stride 258):
        // tgt = out where positive, else NaN; gv = gout; dz0 = (+0 gamma_L) / sd_L; rows beyond the cloud: NaN and +0
        {
            const size_t ob = ((size_t)b * a.N + p0) * cout;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int sl = wave + s * kWaves;
                dz0[s] = 0.0f;
                S[s][0] = tgt[s][0] = gv[s][0] = f32x16{0};
                if (sl * 32 >= cout) continue;  // wave-uniform
                const int oc = min(sl * 32 + j, cout - 1);
                dz0[s] = (0.0f * cl.bn.g[oc]) / sqrtf(cl.bn.v[oc] + kBnEps);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int p = mfma_row(r, h);
                    float ov = nan, g = 0.0f;
                    if (p < nvalid) {
                        ov = a.out[ob + (size_t)p * cout + oc];
                        g = a.gout[ob + (size_t)p * cout + oc];
                    }
                    tgt[s][0][r] = ov > 0.0f ? ov : nan;
                    gv[s][0][r] = g;
                }
            }
        }
        for (int k = 0; k < a.K; ++k) {
            gather_rows<T>(rows, LD, xb, ib, F, a.N, a.K, k, p0, nvalid);
            __syncthreads();
            const float *src = hidden_fwd_chain<LD, 1>(a, lds, F, L);
            // dz_L to its image, d_L against a_{L-1}
            if constexpr (kTrain) {
                last_compare<LD, 1, NS, false>(src, dzl, cl, cinl, cout, wave, h, j, tgt, gv, dz0,
                                               [&](int sl, const f32x16(&)[1], const f32x16(&)[1], const f32x16(&g)[1]) {
                                                   take<LD, NT, NS>(H, hl, g[0], sl, wave, nvalid, basel, src, cinl, h, j);
                                               },
                                               mode_of(a, nvalid), stat_offset(a.w, L));
            } else {
                last_compare<LD, 1, NS, false>(src, dzl, cl, cinl, cout, wave, h, j, tgt, gv, dz0, [&](int sl, const f32x16(&d)[1]) {
                    take<LD, NT, NS>(H, hl, d[0], sl, wave, nvalid, basel, src, cinl, h, j);
                });
            }
            __syncthreads();
            // the way back: d_{l-1} into a_{l-1}'s place and against a_{l-2}
#pragma unroll
            for (int l = kMaxLayers; l >= 2; --l) {
                if (l > L || l <= lmin) continue;  // block-uniform
                const float *ain = l == 2 ? rows : lds + (l - 2) * IMG;
                const int cprev = l == 2 ? 2 * F : a.w[l - 2];
                if constexpr (kTrain) {
                    back_layer<LD, 1>(a, lds, dzl, L, l,
                                      [&](int, int sl, const f32x16(&)[1], const f32x16(&)[1], const f32x16(&g)[1]) {
                                          take<LD, NT, NS>(H, hh[l - 2], g[0], sl, wave, nvalid, base[l - 2] - t0, ain, cprev, h, j);
                                      },
                                      mode_of(a, nvalid));
                } else {
                    back_layer<LD, 1>(a, lds, dzl, L, l, [&](int, int sl, const f32x16(&d)[1]) {
                        take<LD, NT, NS>(H, hh[l - 2], d[0], sl, wave, nvalid, base[l - 2] - t0, ain, cprev, h, j);
                    });
                }
                if (l == L && L >= 3) {  // dz_L is consumed: the edge rows of this k again, for d_1
                    gather_rows<T>(rows, LD, xb, ib, F, a.N, a.K, k, p0, nvalid);
                    __syncthreads();
                }
            }
            if (sums) add_d0<LD, 1, NS>(a, lds, F, wave, h, j, S);
            // (img[1] and `rows` are written again after barriers that a wave reaches after these reads)
        }
        if (sums) {
            store_gx<LD, 1, NS>(a, rows, b, p0, nvalid, wave, h, j, S);
            __syncthreads();  // before the next tile's gather
        }
    }

    // the flush: this pass's tiles of the wave's list, and in pass 0 the h chains (half-wave 0's plus half-wave 1's)
    float *part = a.part + ((size_t)b * gridDim.x + chunk) * a.psize;
#pragma unroll
    for (int i = 0; i < kMaxLayers; ++i) {
        if (i >= L) continue;
        const int ci_w = i == 0 ? 2 * F : a.w[i], co_w = a.w[i + 1];
        const int nci = (ci_w + 31) / 32;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int sl = wave + s * kWaves;
            if (sl * 32 >= co_w) continue;  // wave-uniform
            const int o = sl * 32 + j;
            if (blockIdx.z == 0) {
                float own = hl[s];
                if (i < kMaxLayers - 1 && i + 1 < L) own = hh[i < kMaxLayers - 1 ? i : 0][s];
                const float other = __shfl_xor(own, 32, 64);
                if (h == 0 && o < co_w) part[a.boff[i] + o] = own + other;
            }
            const int tf = base[i] - t0 + s * nci;  // the slab's first tile among this pass's
#pragma unroll
            for (int q = 0; q < NT; ++q) {
                const int ci = q - tf;
                if (ci < 0 || ci >= nci) continue;  // wave-uniform
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int c = ci * 32 + mfma_row(r, h);
                    if (c < ci_w && o < co_w) part[a.woff[i] + c + (size_t)ci_w * o] = H[q][r];
                }
            }
        }
    }
}

struct FinishArgs {
    const float *part;  // (psize, nparts)
    float *sums;        // psize: H_l in W_l's place, h_l in b_l's
    float *g;           // psize: the result
    Conv c[kMaxLayers];
    int woff[kMaxLayers], cin[kMaxLayers], cout[kMaxLayers];
    int nl, psize, nparts;
};

// which layer element e of the parameter buffer belongs to, and its place in the layer's block W | b | gamma | beta | mu | var
__device__ __forceinline__ bool locate(const FinishArgs &f, int e, int *layer, int *at) {
#pragma unroll
    for (int l = 0; l < kMaxLayers; ++l) {
        if (l >= f.nl) break;
        const int n = f.cin[l] * f.cout[l] + 5 * f.cout[l];
        if (e >= f.woff[l] && e < f.woff[l] + n) {
            *layer = l;
            *at = e - f.woff[l];
            return true;
        }
    }
    return false;
}

// ---- the host side -------------------------------------------------------------------------------------------------
struct Plan {
    int ld, nt_w0, passes;  // the row stride; the tiles of wave 0's list (the longest); the passes over it
    unsigned int lmin;      // PgradArgs::lmin
    size_t lds_bytes;
};
// the H tiles a wave keeps in registers: what leaves the kernel without scratch at one wave per SIMD
constexpr int kTilesNarrow = 14, kTilesWide = 12;  // strides 66 and 130 (one slab per wave); stride 258 (two)
// (the training-mode instantiation keeps fewer: narrow, wide are its own)
inline Plan plan(const int32_t *layers, int nlayers, int narrow = kTilesNarrow, int wide = kTilesWide) {
    Plan p{};
    p.ld = adjoint_stride(layers, nlayers);
    const int L = nlayers - 1, nimg = L == 1 ? 2 : L == 2 ? 3 : L;
    p.lds_bytes = (size_t)nimg * 32 * p.ld * sizeof(float);
    for (int i = 1; i < nlayers; ++i) {
        const int cin = i == 1 ? 2 * layers[0] : layers[i - 1];
        p.nt_w0 += (((layers[i] + 31) / 32 + kWaves - 1) / kWaves) * ((cin + 31) / 32);
    }
    const int nt = p.ld == 258 ? wide : narrow;
    p.passes = (p.nt_w0 + nt - 1) / nt;
    // the lowest layer of each pass: that of tile z nt of a wave's list (layer by layer, ascending), over the waves that have one
    for (int z = 0; z < p.passes; ++z) {
        int lmin = nlayers - 1;
        for (int w = 0; w < kWaves; ++w) {
            int at = 0;
            for (int i = 1; i < nlayers; ++i) {
                const int cin = i == 1 ? 2 * layers[0] : layers[i - 1];
                const int slabs = (layers[i] + 31) / 32 - w;
                at += (slabs > 0 ? (slabs + kWaves - 1) / kWaves : 0) * ((cin + 31) / 32);
                if (at > z * nt) {
                    lmin = i < lmin ? i : lmin;
                    break;
                }
            }
        }
        p.lmin |= (unsigned int)lmin << (4 * z);
    }
    return p;
}

// the workspace: the adjoints' prefix (edgeconv_adjoint_plan, with the checks of the entry `fn`) | the chunk partials | the sums
struct WsPlan { AdjointWs adj; size_t part, sums, total; long long psize; int chunks; };
inline fx3d_status ws_plan(const char *fn, const int32_t *layers, int nlayers, int N, int B, int K, WsPlan *w) {
    WsBump ws;
    const fx3d_status rc = edgeconv_adjoint_plan(fn, layers, nlayers, N, B, K, ws, &w->adj);
    if (rc != FX3D_OK) return rc;
    w->psize = edgeconv_layout(nullptr, layers, nlayers, nullptr);
    w->chunks = (N + kGradChunk - 1) / kGradChunk;
    w->part = ws.put((size_t)w->psize * w->chunks * B * sizeof(float));
    w->sums = ws.put((size_t)w->psize * sizeof(float));
    w->total = ws.at;
    return FX3D_OK;
}

// what an entry fills in once the chain's arguments stand in a (edgeconv_adjoint_prepare): where the kernel's partials go and
// where W_l and b_l are, for the kernel and for the finishing kernels (f.g is the entry's own)
inline void pgrad_fill(const float *params_dev, const int32_t *layers, int nlayers, const WsPlan &w, const Plan &p, int B, void *ws,
                       PgradArgs *a, FinishArgs *f) {
    char *wsb = static_cast<char *>(ws);
    const int L = nlayers - 1;
    for (int l = 0; l < L; ++l) {
        a->woff[l] = (int)(a->c[l].W - params_dev);
        a->boff[l] = (int)(a->c[l].b - params_dev);
        f->c[l] = a->c[l];
        f->woff[l] = a->woff[l];
        f->cin[l] = l == 0 ? 2 * layers[0] : layers[l];
        f->cout[l] = layers[l + 1];
    }
    a->psize = (int)w.psize;
    a->part = reinterpret_cast<float *>(wsb + w.part);
    a->lmin = p.lmin;
    f->part = a->part;
    f->sums = reinterpret_cast<float *>(wsb + w.sums);
    f->nl = L; f->psize = a->psize; f->nparts = w.chunks * B;
}

template <int LD, int NS, int NT, class Args>
fx3d_status launch_pgrad(const Args &a, const Plan &p, int chunks, int B, hipStream_t st, const char *label) {
    const void *fn = reinterpret_cast<const void *>(&edgeconv_pgrad_kernel<LD, NS, NT, Args>);
    const fx3d_status rc = ensure_dynamic_lds(fn, (int)kMaxLds, "edgeconv_pgrad_kernel");
    if (rc != FX3D_OK) return rc;
    ProfileScope prof(label, st);
    hipLaunchKernelGGL((edgeconv_pgrad_kernel<LD, NS, NT, Args>), dim3(chunks, B, p.passes), dim3(kPtThreads), p.lds_bytes, st, a);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

// sums[e] = the chain from +0 over the chunk partials f.part, b ascending, chunk ascending, for the elements of every H_l and h_l
// (edgeconv_pgrad.hip: pgrad_reduce)
fx3d_status launch_pgrad_reduce(const FinishArgs &f, hipStream_t st);

}  // namespace mlp
}  // namespace fx3d
