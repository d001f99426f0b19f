// Feature-space k-NN on the matrix cores (4 <= D <= 128): the per-cloud pre-pass of fx3d_knn_ws and knn_mfma_kernel -- one
// translation unit of the k-NN family (knn_common.h).
#include "knn_common.h"

namespace {

// ------------------------------------------------------------------------------------------------
// knn_mfma_kernel<DK, MODE>: feature-space kNN (4 <= D <= 128, k+drop <= 32; the second EdgeConv runs at D = 64).
// Same selection scheme as knn_f16_d3_kernel (lane = query; 64 group minima -> tau in registers; per-lane mask
// lists; verified distance-only ranking), with the filter as a dense Float32 GEMM:
//   F[c][q] = fl(|c|^2) + sum_d c_d (-2 q_d)   on v_mfma_f32_32x32x2_f32 (rows = 32 candidates of a tile, columns
//   = the wave's 32 queries, the accumulator starts at |c|^2; two tiles on two accumulators).  With u = 2^-24 and
//   the usual gamma_n bounds, |F + |q|^2 - d_oracle| <= eps_q = 8 (D+4) u (|q|^2 + Cmax^2) for every candidate
//   (Cmax = largest candidate norm of the cloud; 2x head-room for the matrix core's internal rounding), so the
//   candidates with F <= tau + 2 eps_q are a superset of the k nearest.
// Block = 4 consumer waves (32 queries each) + 4 producer waves that stage the next candidate chunk into the other
// LDS buffer with global_load_lds_dwordx4 while the consumers work (one consumer wave per SIMD: nothing else
// would hide global latency; VALU work of any wave delays that SIMD's MFMAs, hence the direct loads).  The
// reduction dimension is permuted so that half-wave h owns d in [h*DP/2, (h+1)*DP/2): every operand fetch is a
// b128 (4 k-steps); the LDS image is lane-linear, the conflict-free rotation sits on the source addresses.
// In the exact phase all eight waves work: the four lanes of a query (two halves x consumer/producer) split its
// survivors; candidate and query rows are gathered from L2.
// Modes (KnnFilter): F32: the Float32 GEMM above.  F16 / F16Pre (default for D % 4 == 0, M <= 4096): the cloud is
// centred per dimension and scaled by a power of two, operands are the rounded fp16 halves (one v_mfma_f32_32x32x16_f16
// per K block, band 2^-10 (|q~|^2 + C~max^2)).  Producers convert while staging.
// Queries whose band holds more candidates than the key arrays (60) but whose lane lists are intact take the medium
// path (exact selection among their own survivors, up to kMMedCap); the rest of the leftovers the full exact merge.
// Behind the pre-pass (fx3d_knn_ws: the cloud's fp16 image, norms and header exist in the workspace) both waves of a pair run the
// filter (128 group minima per query), every lane reads its pieces of its query row and of the centre straight from memory, the
// image chunks come through registers (D <= 64) or by the producers' direct-to-LDS loads, phase A folds two tiles per v_min3 on
// the MFMA registers, phase B starts the accumulators at n_c - thr and shifts the signs in with v_alignbit, and tau comes from
// knn_tau_8of16.
// The kernel is a sequence of phases, one function each, in file order: block and lane coordinates (knn_mfma_coords) | scale pass
// or header read (knn_mfma_scale) | query operand | first chunk | chunk loop: per step the filter of the resident chunk and the
// staging of the next (knn_mfma_chunk_step) | tau and threshold | list counts and path flags | medium path | decode | exact
// distances: 16-dimension COLUMN SLICES of the whole cloud (M <= 1024, D % 16 == 0, D <= 64), row stages (D > 64: in two column
// halves) or a gather from L2, chosen by shape in knn_mfma_plan | rank | output | leftover merge.  The phases share KnnMfmaCtx (the
// arguments, the LDS regions of KnnMfmaLds, the thread's coordinates); the mode is one template parameter (KnnFilter), and each
// mode decision sits in the one function that owns it.  How the kernel got here, with the measurements: DESIGN.md 3.2.
constexpr int kMLCap = 40;        // rows of a lane's mask list (39 usable + the scratch head)
constexpr int kMKeyCap = 64;      // survivors per query handled by the fast path (three sentinels follow them inside the stride of 68)
constexpr int kMMedCap = 512;     // ... by the medium path: exact selection among the query's own survivors
constexpr int kMKeyStride = 68;   // row stride of the key arrays in words: 32 queries x b128 reads without bank conflicts

// fp16 staging of a candidate chunk (producer side, F16 filter): unit = (row, group of 8 dimensions).
// A thread converts two float4 of a row (scaled by sc) into one piece of 8 halves.
// (row, group) units per producer thread and chunk: CH * (DP/8) <= kMUnits * 256, which bounds the chunk length (long
// chunks mean fewer steps: a step cannot be shorter than the latency of the global loads issued one step ahead)
constexpr int kMUnits = 6;
template <int DK>
__device__ __forceinline__ void knn_f16_load_chunk(const float *__restrict__ yb, int D, int j0, int cn, int CH, int ptid,
                                                   float4 (&reg)[kMUnits][2]) {
    constexpr int DP = DK * 32, G = DP / 8;
    // unconditional loads from clamped (always valid) addresses, zeroed afterwards: predicated loads would be
    // issued one branch at a time, each waiting for its data
    const float4 zero4 = float4{0.f, 0.f, 0.f, 0.f};
    const int cnm1 = cn - 1;
#pragma unroll
    for (int u = 0; u < kMUnits; ++u) {
        const int un = ptid + u * kMProd;
        const int row = un / G, g = un - row * G;
        const int rowc = row < cnm1 ? row : cnm1;
        const int d0 = 8 * g < D ? 8 * g : 0, d1 = 8 * g + 4 < D ? 8 * g + 4 : 0;
        const float *src = yb + (size_t)(j0 + rowc) * D;
        reg[u][0] = *reinterpret_cast<const float4 *>(src + d0);
        reg[u][1] = *reinterpret_cast<const float4 *>(src + d1);
    }
#pragma unroll
    for (int u = 0; u < kMUnits; ++u) {
        const int un = ptid + u * kMProd;
        const int row = un / G, g = un - row * G;
        const bool ok = un < CH * G && row < cn;
        if (!(ok && 8 * g < D)) reg[u][0] = zero4;
        if (!(ok && 8 * g + 4 < D)) reg[u][1] = zero4;
    }
}
// fp16 image: rows of PPI = DP/8 pieces (16 bytes = 8 halves); piece c of row r sits
// at (c + r / RPB) mod PPI, RPB = rows per 256 bytes, so that 16 consecutive rows cover all LDS banks.
template <int PPI>
__device__ __forceinline__ int knn_hpiece_off(int row, int c) {
    constexpr int RPB = PPI >= 16 ? 1 : 16 / PPI;
    return (row * PPI + ((c + row / RPB) & (PPI - 1))) * 4;
}
// Converts and stores the units; the G = DP/8 consecutive lanes that hold one row also sum its scaled norm
// (3..4 butterfly steps).  norms != nullptr: phase A, norms[row] and the running maximum are recorded.
template <int CTRL>
__device__ __forceinline__ float knn_dpp(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
template <int DK>
__device__ __forceinline__ void knn_f16_store_chunk(float *img, int CH, int cn, float sc, const float *mu_lds, int ptid,
                                                    const float4 (&reg)[kMUnits][2], float *norms, float *norms_m,
                                                    const float *acoef_lds, float &tmax, bool &tnan) {
    constexpr int DP = DK * 32, G = DP / 8;
    static_assert(kMProd % G == 0, "a producer thread always converts the same group of eight dimensions");
    static_assert(G == 4 || G == 8 || G == 16, "the row sum below");
    // (centre and error coefficient are re-read from LDS per call: holding them in registers across the chunk loop spills)
    float mu8[8];
    {
        const float4 m0 = *reinterpret_cast<const float4 *>(mu_lds + 8 * (ptid % G)), m1 = *reinterpret_cast<const float4 *>(mu_lds + 8 * (ptid % G) + 4);
        mu8[0] = m0.x; mu8[1] = m0.y; mu8[2] = m0.z; mu8[3] = m0.w; mu8[4] = m1.x; mu8[5] = m1.y; mu8[6] = m1.z; mu8[7] = m1.w;
    }
    const float acoef = norms_m ? *acoef_lds : 0.0f;
#pragma unroll
    for (int u = 0; u < kMUnits; ++u) {
        const int un = ptid + u * kMProd;
        const int row = un / G, g = un - row * G;
        const float v[8] = {(reg[u][0].x - mu8[0]) * sc, (reg[u][0].y - mu8[1]) * sc, (reg[u][0].z - mu8[2]) * sc,
                            (reg[u][0].w - mu8[3]) * sc, (reg[u][1].x - mu8[4]) * sc, (reg[u][1].y - mu8[5]) * sc,
                            (reg[u][1].z - mu8[6]) * sc, (reg[u][1].w - mu8[7]) * sc};
        kh8 hi;
        float part = 0.0f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            hi[e] = (_Float16)v[e];
            part = __builtin_fmaf(v[e], v[e], part);
        }
        if (un < CH * G) *reinterpret_cast<kh8 *>(img + knn_hpiece_off<G>(row, g)) = hi;
        if (norms) {  // wave-uniform
            // sum over the row's G lanes by DPP (VALU speed; the same tree as an xor butterfly in the row's first lane,
            // the only one that uses it)
            part = part + knn_dpp<0xB1>(part);                // quad_perm [1,0,3,2]
            part = part + knn_dpp<0x4E>(part);                // quad_perm [2,3,0,1]
            if (G >= 8) part = part + knn_dpp<0x141>(part);   // row_half_mirror
            if (G >= 16) part = part + knn_dpp<0x140>(part);  // row_mirror
            if (un < CH * G && g == 0) {
                const float t = row < cn ? part : INFINITY;  // rows beyond the cloud: F = +inf
                // norms_m: the candidate's own share of the filter error is folded into its norm, upwards for the
                // threshold search (phase A), downwards for the test (phase B)
                norms[row] = norms_m ? t + acoef * t : t;
                if (norms_m) norms_m[row] = row < cn ? t - acoef * t : INFINITY;
                if (row < cn) { tnan |= (t != t); tmax = fmaxf(tmax, t); }
            }
        }
    }
}

// staged exact phase: the oracle's squared distance of one query row (registers) to two staged candidate rows (LDS),
// dimension by dimension in order.  Differences and squares two dimensions per instruction (v_pk_add/mul_f32 on the
// natural register pairs), the sums one by one; the next four pieces of both rows are in flight while four are summed.
// FULL: D == DP (no guards).
template <int DP, bool FULL>
__device__ __forceinline__ void knn_pair_dist(const f32x4v (&q)[DP / 4], const float *cp0, const float *cp1, int D, float &s0, float &s1) {
    constexpr int NB = DP / 16;
    f32x4v c0[2][4], c1[2][4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (FULL || 4 * t < D) {
            c0[0][t] = *reinterpret_cast<const f32x4v *>(cp0 + 4 * t);
            c1[0][t] = *reinterpret_cast<const f32x4v *>(cp1 + 4 * t);
        }
#pragma unroll
    for (int bk = 0; bk < NB; ++bk) {
        if (bk + 1 < NB) {
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (FULL || 16 * (bk + 1) + 4 * t < D) {
                    c0[(bk + 1) & 1][t] = *reinterpret_cast<const f32x4v *>(cp0 + 16 * (bk + 1) + 4 * t);
                    c1[(bk + 1) & 1][t] = *reinterpret_cast<const f32x4v *>(cp1 + 16 * (bk + 1) + 4 * t);
                }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (FULL || 16 * bk + 4 * t < D) {
                const f32x4v d0 = q[4 * bk + t] - c0[bk & 1][t], d1 = q[4 * bk + t] - c1[bk & 1][t];
                const f32x4v m0 = d0 * d0, m1 = d1 * d1;
                s0 = s0 + m0.x; s0 = s0 + m0.y; s0 = s0 + m0.z; s0 = s0 + m0.w;
                s1 = s1 + m1.x; s1 = s1 + m1.y; s1 = s1 + m1.z; s1 = s1 + m1.w;
            }
    }
}

// staged exact phase: a thread's share of one stage of candidate rows (8 pieces of 16 bytes, rows srow + i * RPI of
// the stage that starts at row g0; clamped addresses: always valid, unused rows are never stored)
__device__ __forceinline__ void knn_stage_fetch(const float *__restrict__ yb, int D, int M, int g0, int srow, int RPI, int scol,
                                                f32x4v (&reg)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        int g = g0 + srow + i * RPI;
        g = g < M ? g : M - 1;
        reg[i] = *reinterpret_cast<const f32x4v *>(yb + (size_t)g * D + scol);
    }
}

// LDS image of a chunk: rows of PPR = DP/4 16-byte pieces, no padding; piece c of row r sits at position
// (c + r) mod PPR of its row.  The rotation makes the consumers' b128 operand fetches (32 consecutive rows, one
// column) conflict-free, and it is applied on the SOURCE side of the direct-to-LDS loads
// (global_load_lds_dwordx4 writes lane-linear: wave-uniform base + lane*16), so staging costs one
// instruction per KiB and no VGPR round trip -- the producers share their SIMD's issue slots with the
// consumers' MFMAs, every VALU instruction they do not execute is matrix-core time.
template <int DK>
__device__ __forceinline__ int knn_piece_off(int row, int c) {  // float offset of piece c of row `row`
    constexpr int PPR = DK * 8;
    return (row * PPR + ((c + row) & (PPR - 1))) * 4;
}

// producer wave pw stages rows [pw*RW, (pw+1)*RW) of the chunk [j0, j0+cn) and their norms
template <int DK>
__device__ __forceinline__ void knn_stage_chunk(const float *__restrict__ yb, int D, int j0, int cn, int CH, float *img,
                                                float *cnorm, unsigned int *cmax, bool want_cmax, bool do_norms,
                                                bool vec4, int pw, int lane) {
    constexpr int PPR = DK * 8;
    const int RW = CH / kMWaves;          // rows per producer wave (CH is a multiple of 64)
    const int row_lo = pw * RW;
    const int rq = D / 4;
    if (vec4) {
        const int ninstr = RW * PPR / 64;
        for (int i = 0; i < ninstr; ++i) {
            const int S0 = row_lo * PPR + i * 64;  // first 16-byte slot of this wave-instruction
            const int S = S0 + lane;
            const int row = S / PPR, pos = S & (PPR - 1);
            const int c = (pos - row) & (PPR - 1);
            if (row < cn && c < rq)
                __builtin_amdgcn_global_load_lds(
                    (const __attribute__((address_space(1))) void *)(yb + (size_t)(j0 + row) * D + 4 * c),
                    (__attribute__((address_space(3))) void *)(img + (size_t)S0 * 4), 16, 0, 0);
        }
        __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0): this wave's pieces have landed
    } else {
        for (int e = lane; e < RW * D; e += 64) {
            const int row = row_lo + e / D, d = e % D;
            if (row < cn) img[knn_piece_off<DK>(row, d >> 2) + (d & 3)] = yb[(size_t)(j0 + row) * D + d];
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);
    }
    __builtin_amdgcn_wave_barrier();
    if (!do_norms) return;  // phase B with the norms of phase A kept in LDS
    // norms of this wave's rows (padding columns hold zeros); rows beyond the chunk get +inf: F = +inf
    float wmax = 0.0f;
    bool wnan = false;
    for (int r0 = 0; r0 < RW; r0 += 64) {
        const int row = row_lo + r0 + lane;
        if (r0 + lane < RW) {
            float t = INFINITY;
            if (row < cn) {
                t = 0.0f;
#pragma unroll
                for (int c = 0; c < PPR; ++c) {
                    const float4 v = *reinterpret_cast<const float4 *>(img + knn_piece_off<DK>(row, c));
                    t = __builtin_fmaf(v.x, v.x, t);
                    t = __builtin_fmaf(v.y, v.y, t);
                    t = __builtin_fmaf(v.z, v.z, t);
                    t = __builtin_fmaf(v.w, v.w, t);
                }
                wnan |= (t != t);
                wmax = fmaxf(wmax, t);
            }
            cnorm[row] = t;
        }
    }
    if (want_cmax) {
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) wmax = fmaxf(wmax, __shfl_xor(wmax, m, 64));
        const bool anynan = __ballot(wnan) != 0;
        if (lane == 0) atomicMax(cmax, anynan ? 0x7fc00000u : __builtin_bit_cast(unsigned int, wmax));  // NaN > +inf
    }
}

// ------------------------------------------------------------------------------------------------
// Pre-pass of the feature-space kNN (fx3d_knn_ws): the per-cloud statistics and the fp16 image are built ONCE per cloud
// instead of by every block of the cloud (8 blocks per cloud at C4': the scale pass alone was 8 us of the 78, bound by the
// L2 -- every block read the whole cloud -- and the producers' conversion VALU delayed the consumers' MFMAs in both phases).
//   knn_pre_stats_kernel   grid (kPreParts * B): minima / maxima / sums per dimension of one eighth of the cloud's rows
//   knn_pre_image_kernel   grid (kPreParts * B): combines the eight parts (every block the same arithmetic: identical centre
//                          and scale), robust centre as in knn_mfma_kernel, converts its rows: fp16 image [Mpad][DP], scaled
//                          row norms (the candidate's error share folded in, upwards / downwards), largest norm of the part
// knn_mfma_kernel then reads the header, and its producer waves bring image chunks and norms in with direct-to-LDS loads (no
// VALU).  Workspace per cloud: KnnPre::cloud_bytes(M, DP).
constexpr int kPreParts = 8;
constexpr int kPreThreads = 256;
struct KnnPre {
    unsigned char *base;  // workspace
    size_t stride;        // bytes per cloud
    int Mpad;             // rows of the image (multiple of 256: chunks never need a clamp), DP halves per row
    // offsets inside a cloud's slab (bytes)
    size_t off_parts, off_hdr, off_cmax, off_nup, off_ndn, off_img;
    __host__ __device__ static KnnPre make(void *ws, int M, int DP) {
        KnnPre k{};
        k.base = static_cast<unsigned char *>(ws);
        k.Mpad = (M + 255) / 256 * 256;
        size_t o = 0;
        k.off_parts = o; o += (size_t)kPreParts * (3 * DP + 4) * 4;
        k.off_hdr = o; o += (size_t)(8 + DP) * 4;
        k.off_cmax = o; o += (size_t)kPreParts * 4;
        o = (o + 63) & ~(size_t)63;
        k.off_nup = o; o += (size_t)k.Mpad * 4;
        k.off_ndn = o; o += (size_t)k.Mpad * 4;
        k.off_img = o; o += (size_t)k.Mpad * DP * 2;
        k.stride = (o + 255) & ~(size_t)255;
        return k;
    }
    __host__ __device__ float *parts(int b) const { return reinterpret_cast<float *>(base + (size_t)b * stride + off_parts); }
    __host__ __device__ float *hdr(int b) const { return reinterpret_cast<float *>(base + (size_t)b * stride + off_hdr); }
    __host__ __device__ unsigned int *cmaxp(int b) const { return reinterpret_cast<unsigned int *>(base + (size_t)b * stride + off_cmax); }
    __host__ __device__ float *nup(int b) const { return reinterpret_cast<float *>(base + (size_t)b * stride + off_nup); }
    __host__ __device__ float *ndn(int b) const { return reinterpret_cast<float *>(base + (size_t)b * stride + off_ndn); }
    __host__ __device__ _Float16 *img(int b) const { return reinterpret_cast<_Float16 *>(base + (size_t)b * stride + off_img); }
};
// header floats: [0] sc  [1] funit  [2] acoef (candidate side)  [3] bits: 1 = non-finite / overflow-prone cloud  [8 ...] mu[DP]

// The parts' statistics travel between the blocks of a cloud INSIDE the fused pre-pass kernel: device-coherent accesses (relaxed
// atomics at agent scope: write-through stores, loads that do not hit a stale line -- the blocks may sit on different XCDs, each
// with its own L2) instead of agent-scope fences, which write back / invalidate a whole L2 per block (measured: + 0.1 us per block
// of the grid, serialised per XCD: C4' 76 -> 104 us).
__device__ __forceinline__ void knn_pre_put(float *p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float knn_pre_get(const float *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void knn_pre_stats_body(const float *__restrict__ y, int M, int D, int DP, const KnnPre &pre, int part, int b,
                                                   float *red) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float *yb = y + (size_t)b * M * D;
    const int rq = D / 4;  // (kPreThreads % rq == 0: thread t always sees dimensions 4 (t % rq) ...)
    const int per = (M + kPreParts - 1) / kPreParts;
    const int r_lo = part * per < M ? part * per : M, r_hi = r_lo + per < M ? r_lo + per : M;
    const float4 *c4 = reinterpret_cast<const float4 *>(yb) + (size_t)r_lo * rq;
    const int total4 = (r_hi - r_lo) * rq;
    float4 lo4 = float4{INFINITY, INFINITY, INFINITY, INFINITY}, hi4 = float4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    float4 sum4 = float4{0.f, 0.f, 0.f, 0.f};
    float poison = 0.0f;
    for (int e0 = tid; e0 < total4; e0 += 8 * kPreThreads) {
        float4 v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = c4[e0 + e * kPreThreads < total4 ? e0 + e * kPreThreads : e0];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            poison = __builtin_fmaf(v[e].x, 0.0f, poison); poison = __builtin_fmaf(v[e].y, 0.0f, poison);
            poison = __builtin_fmaf(v[e].z, 0.0f, poison); poison = __builtin_fmaf(v[e].w, 0.0f, poison);
            lo4.x = fminf(lo4.x, v[e].x); lo4.y = fminf(lo4.y, v[e].y); lo4.z = fminf(lo4.z, v[e].z); lo4.w = fminf(lo4.w, v[e].w);
            hi4.x = fmaxf(hi4.x, v[e].x); hi4.y = fmaxf(hi4.y, v[e].y); hi4.z = fmaxf(hi4.z, v[e].z); hi4.w = fmaxf(hi4.w, v[e].w);
            if (e0 + e * kPreThreads < total4) {
                sum4.x = sum4.x + v[e].x; sum4.y = sum4.y + v[e].y; sum4.z = sum4.z + v[e].z; sum4.w = sum4.w + v[e].w;
            }
        }
    }
    const bool anynan = __syncthreads_or(poison != poison) != 0;
    for (int m = rq; m < 64; m <<= 1) {  // lanes with equal lane % rq hold the same dimensions
        lo4.x = fminf(lo4.x, __shfl_xor(lo4.x, m, 64)); lo4.y = fminf(lo4.y, __shfl_xor(lo4.y, m, 64));
        lo4.z = fminf(lo4.z, __shfl_xor(lo4.z, m, 64)); lo4.w = fminf(lo4.w, __shfl_xor(lo4.w, m, 64));
        hi4.x = fmaxf(hi4.x, __shfl_xor(hi4.x, m, 64)); hi4.y = fmaxf(hi4.y, __shfl_xor(hi4.y, m, 64));
        hi4.z = fmaxf(hi4.z, __shfl_xor(hi4.z, m, 64)); hi4.w = fmaxf(hi4.w, __shfl_xor(hi4.w, m, 64));
        sum4.x = sum4.x + __shfl_xor(sum4.x, m, 64); sum4.y = sum4.y + __shfl_xor(sum4.y, m, 64);
        sum4.z = sum4.z + __shfl_xor(sum4.z, m, 64); sum4.w = sum4.w + __shfl_xor(sum4.w, m, 64);
    }
    if (lane < rq) {
        float *r8 = red + (size_t)(wv * 32 + lane) * 12;
        r8[0] = lo4.x; r8[1] = lo4.y; r8[2] = lo4.z; r8[3] = lo4.w;
        r8[4] = hi4.x; r8[5] = hi4.y; r8[6] = hi4.z; r8[7] = hi4.w;
        r8[8] = sum4.x; r8[9] = sum4.y; r8[10] = sum4.z; r8[11] = sum4.w;
    }
    __syncthreads();
    float *out = pre.parts(b) + (size_t)part * (3 * DP + 4);
    if (tid < rq) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float lo = INFINITY, hi = -INFINITY, sm = 0.0f;
            for (int w = 0; w < kPreThreads / 64; ++w) {
                const float *r8 = red + (size_t)(w * 32 + tid) * 12;
                lo = fminf(lo, r8[c]); hi = fmaxf(hi, r8[4 + c]); sm = sm + r8[8 + c];
            }
            knn_pre_put(out + 4 * tid + c, lo); knn_pre_put(out + DP + 4 * tid + c, hi); knn_pre_put(out + 2 * DP + 4 * tid + c, sm);
        }
    }
    if (tid == 0) knn_pre_put(out + 3 * DP, __builtin_bit_cast(float, anynan ? 1 : 0));
}
__global__ __launch_bounds__(kPreThreads) void knn_pre_stats_kernel(const float *__restrict__ y, int M, int D, int DP, KnnPre pre) {
    __shared__ float red[(kPreThreads / 64) * 32 * 12];
    knn_pre_stats_body(y, M, D, DP, pre, blockIdx.x % kPreParts, blockIdx.x / kPreParts, red);
}

// mu: [DP] floats, sh: 4 words of LDS ([0] bits of the extent  [1] skew flag  [2] bits of the bulk radius  [3] largest norm of the part)
template <int DK>
__device__ __forceinline__ void knn_pre_image_body(const float *__restrict__ y, int M, int D, int two_norms, const KnnPre &pre, int part, int b,
                                                   float *mu, unsigned int *sh) {
    constexpr int DP = DK * 32, G = DP / 8;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float *yb = y + (size_t)b * M * D;
    const int rq = D / 4;
    const float *parts = pre.parts(b);
    // this part's rows: the first four sweeps (a whole part at C4': 128 rows) are requested BEFORE the parts' statistics are read --
    // the rows do not depend on them, and the kernel is two dependent global round trips otherwise
    const int per = (M + kPreParts - 1) / kPreParts;
    const int r_lo = part * per < M ? part * per : M, r_hi = r_lo + per < M ? r_lo + per : M;
    const int g = tid % G;  // (kPreThreads % G == 0: a thread always converts the same eight dimensions)
    constexpr int RPS = kPreThreads / G;  // rows per sweep of the block
    const int d0 = 8 * g < D ? 8 * g : 0, d1 = 8 * g + 4 < D ? 8 * g + 4 : 0;
    float4 a0[4], a1[4];
    auto load_rows = [&](int r0) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {  // every load of the four sweeps before the first use (a part is a few sweeps: latency, not bandwidth)
            const int row = r0 + u * RPS + tid / G;
            const float *src = yb + (size_t)(row < r_hi ? row : (r_lo < M ? r_lo : 0)) * D;
            a0[u] = *reinterpret_cast<const float4 *>(src + d0);
            a1[u] = *reinterpret_cast<const float4 *>(src + d1);
        }
    };
    load_rows(r_lo);
    if (tid < 4) sh[tid] = 0u;
    bool anynan = false;
    for (int p = 0; p < kPreParts; ++p) anynan |= __builtin_bit_cast(int, knn_pre_get(parts + (size_t)p * (3 * DP + 4) + 3 * DP)) != 0;
    __syncthreads();
    if (tid < rq) {
        float amax = 0.0f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float lo = INFINITY, hi = -INFINITY, sm = 0.0f;
            for (int p = 0; p < kPreParts; ++p) {  // (fixed order: every block of the cloud gets the same centre)
                const float *q = parts + (size_t)p * (3 * DP + 4);
                lo = fminf(lo, knn_pre_get(q + 4 * tid + c)); hi = fmaxf(hi, knn_pre_get(q + DP + 4 * tid + c)); sm = sm + knn_pre_get(q + 2 * DP + 4 * tid + c);
            }
            float m0 = sm / (float)M;
            m0 = fminf(fmaxf(m0, lo), hi);
            mu[4 * tid + c] = m0;
            amax = fmaxf(amax, fmaxf(hi - m0, m0 - lo));
            if (fabsf(m0 - 0.5f * (lo + hi)) > 0.25f * (hi - lo)) sh[1] = 1u;
        }
        atomicMax(&sh[0], __builtin_bit_cast(unsigned int, amax));
    } else if (tid < DP / 4) {
        mu[4 * tid] = 0.0f; mu[4 * tid + 1] = 0.0f; mu[4 * tid + 2] = 0.0f; mu[4 * tid + 3] = 0.0f;
    }
    __syncthreads();
    if (sh[1] != 0u && !anynan) {  // robust centre: see knn_mfma_kernel (the same rule on the same 16 sampled rows)
        if (wv == 0) {
            float shiftmax = 0.0f, iqr2 = 0.0f;
            bool sw = false;
            float medv[DP / 64 > 0 ? DP / 64 : 1];
#pragma unroll
            for (int t = 0; t < (DP + 63) / 64; ++t) {
                const int d = lane + 64 * t;
                float v[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) v[i] = yb[(size_t)((long long)i * M / 16) * D + (d < D ? d : 0)];
                float med = v[0], q1 = v[0], q3 = v[0];
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    int rk = 0;
#pragma unroll
                    for (int j = 0; j < 16; ++j) rk += (v[j] < v[i] || (v[j] == v[i] && j < i)) ? 1 : 0;
                    med = rk == 8 ? v[i] : med; q1 = rk == 4 ? v[i] : q1; q3 = rk == 12 ? v[i] : q3;
                }
                const float shift = d < D ? fabsf(mu[d < D ? d : 0] - med) : 0.0f;
                sw = sw || (shift > 8.0f * (q3 - q1));
                shiftmax = fmaxf(shiftmax, shift);
                if (d < D) iqr2 = __builtin_fmaf(q3 - q1, q3 - q1, iqr2);
                medv[t] = med;
            }
            if (__ballot(sw) != 0ull) {
#pragma unroll
                for (int m = 1; m < 64; m <<= 1) {
                    shiftmax = fmaxf(shiftmax, __shfl_xor(shiftmax, m, 64));
                    iqr2 = iqr2 + __shfl_xor(iqr2, m, 64);
                }
#pragma unroll
                for (int t = 0; t < (DP + 63) / 64; ++t)
                    if (lane + 64 * t < D) mu[lane + 64 * t] = medv[t];
                if (lane == 0) {
                    sh[0] = __builtin_bit_cast(unsigned int, __builtin_bit_cast(float, sh[0]) + shiftmax);
                    sh[2] = __builtin_bit_cast(unsigned int, sqrtf(iqr2));
                }
            }
        }
        __syncthreads();
    }
    const float cinf = __builtin_bit_cast(float, sh[0]);
    float sc = 1.0f;
    if (cinf > kTinyExtent && cinf < 1.0e30f) {
        int e;
        (void)frexpf(cinf * 1.000001f, &e);
        sc = ldexpf(1.0f, 10 - e);
    }
    const float rad = __builtin_bit_cast(float, sh[2]);
    const float funit = rad > 0.0f ? fminf(1.0f, fmaxf(sc * rad, 0x1p-12f)) : 1.0f;
    const float aq = 8.0f * (float)(4 * D + 8) * 0x1p-24f + 0x1.01p-10f;
    const float acoef = aq * 1.01f + 0x1p-26f * sqrtf((float)D) / funit + 0x1p-23f;
    const bool bad = anynan || !(cinf < 1.0e15f);
    if (part == 0) {
        float *h = pre.hdr(b);
        if (tid == 0) { h[0] = sc; h[1] = funit; h[2] = acoef; h[3] = bad ? 1.0f : 0.0f; }
        if (tid < DP) h[8 + tid] = mu[tid];
    }
    // ---- this part's rows -> image, norms
    _Float16 *img = pre.img(b);
    float *nup = pre.nup(b), *ndn = pre.ndn(b);
    float mu8[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) mu8[e] = mu[8 * g + e];
    float tmax = 0.0f;
    bool tnan = false;
    for (int r0 = r_lo; r0 < r_hi; r0 += 4 * RPS) {
        if (r0 != r_lo) load_rows(r0);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int row = r0 + u * RPS + tid / G;
            const bool ok = row < r_hi;
            if (!(8 * g < D)) a0[u] = float4{mu8[0], mu8[1], mu8[2], mu8[3]};       // padding dimensions: zero pieces
            if (!(8 * g + 4 < D)) a1[u] = float4{mu8[4], mu8[5], mu8[6], mu8[7]};
            const float v[8] = {(a0[u].x - mu8[0]) * sc, (a0[u].y - mu8[1]) * sc, (a0[u].z - mu8[2]) * sc, (a0[u].w - mu8[3]) * sc,
                                (a1[u].x - mu8[4]) * sc, (a1[u].y - mu8[5]) * sc, (a1[u].z - mu8[6]) * sc, (a1[u].w - mu8[7]) * sc};
            kh8 hi;
            float pt = 0.0f;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                hi[e] = (_Float16)v[e];
                pt = __builtin_fmaf(v[e], v[e], pt);
            }
            pt = pt + knn_dpp<0xB1>(pt);
            pt = pt + knn_dpp<0x4E>(pt);
            if (G >= 8) pt = pt + knn_dpp<0x141>(pt);
            if (G >= 16) pt = pt + knn_dpp<0x140>(pt);
            if (ok) {
                *reinterpret_cast<kh8 *>(img + ((size_t)row * G + g) * 8) = hi;
                if (g == 0) {
                    nup[row] = two_norms ? pt + acoef * pt : pt;
                    ndn[row] = two_norms ? pt - acoef * pt : pt;
                    tnan |= (pt != pt);
                    tmax = fmaxf(tmax, pt);
                }
            }
        }
    }
    if (part == kPreParts - 1) {  // rows [M, Mpad): zero pieces, norm +inf (F = +inf: never selected)
        kh8 z;
#pragma unroll
        for (int e = 0; e < 8; ++e) z[e] = (_Float16)0.0f;
        for (int un = tid; un < (pre.Mpad - M) * G; un += kPreThreads) *reinterpret_cast<kh8 *>(img + ((size_t)M * G + un) * 8) = z;
        for (int r = M + tid; r < pre.Mpad; r += kPreThreads) { nup[r] = INFINITY; ndn[r] = INFINITY; }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) tmax = fmaxf(tmax, __shfl_xor(tmax, m, 64));
    const bool anyn = __ballot(tnan) != 0;
    if (lane == 0) atomicMax(&sh[3], anyn ? 0x7fc00000u : __builtin_bit_cast(unsigned int, tmax));
    __syncthreads();
    if (tid == 0) pre.cmaxp(b)[part] = bad ? 0x7fc00000u : sh[3];
}
template <int DK>
__global__ __launch_bounds__(kPreThreads) void knn_pre_image_kernel(const float *__restrict__ y, int M, int D, int two_norms, KnnPre pre) {
    __shared__ float mu[DK * 32];
    __shared__ unsigned int sh[4];
    knn_pre_image_body<DK>(y, M, D, two_norms, pre, blockIdx.x % kPreParts, blockIdx.x / kPreParts, mu, sh);
}
// (Two launches: one 1024-thread block per cloud for the whole pre-pass measured slower)

// producer wave pw brings the norms of chunk [j0, j0 + CH) into the block's norm arrays (direct-to-LDS; not waited for here)
__device__ __forceinline__ void knn_pre_stage_norms(const float *__restrict__ gnup, const float *__restrict__ gndn, int j0, int CH, float *nup,
                                                    float *ndn, int pw, int lane) {
    const int nin = CH / 4 / 64;  // wave-instructions per norm array (CH / 4 pieces of four floats); CH = 64 -> a quarter wave
    for (int i = pw; i < (nin > 0 ? nin : 1); i += kMWaves)
        if (i * 64 + lane < CH / 4) {
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(gnup + j0 + (size_t)(i * 64 + lane) * 4),
                                             (__attribute__((address_space(3))) void *)(nup + (size_t)i * 256), 16, 0, 0);
            if (ndn)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(gndn + j0 + (size_t)(i * 64 + lane) * 4),
                                                 (__attribute__((address_space(3))) void *)(ndn + (size_t)i * 256), 16, 0, 0);
        }
}
// producer wave pw brings chunk [j0, j0 + CH) of the pre-pass image into `img` (the layout of knn_hpiece_off: the
// rotation sits on the source address) and, in phase A, its norms into the block's norm arrays -- direct-to-LDS loads only, not
// waited for here
template <int DK>
__device__ __forceinline__ void knn_pre_stage_chunk(const _Float16 *__restrict__ gimg, const float *__restrict__ gnup,
                                                    const float *__restrict__ gndn, int j0, int CH, float *img, float *nup,
                                                    float *ndn, bool norms, int pw, int lane) {
    constexpr int PPI = DK * 4;                       // 16-byte pieces per image row (DP halves)
    constexpr int RPB = PPI >= 16 ? 1 : 16 / PPI;
    const int ninstr = CH * PPI / 64 / kMWaves;       // wave-instructions of this producer wave (CH is a multiple of 64)
    for (int i = 0; i < ninstr; ++i) {
        const int S0 = (pw * ninstr + i) * 64;        // first 16-byte slot of this wave-instruction
        const int S = S0 + lane;
        const int row = S / PPI, pos = S & (PPI - 1);
        const int c = (pos - row / RPB) & (PPI - 1);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(gimg + ((size_t)(j0 + row) * PPI + c) * 8),
                                         (__attribute__((address_space(3))) void *)(img + (size_t)S0 * 4), 16, 0, 0);
    }
    if (norms) knn_pre_stage_norms(gnup, gndn, j0, CH, nup, ndn, pw, lane);
}

// ------------------------------------------------------------------------------------------------
// knn_mfma_kernel: filter modes, arguments, LDS layout, context.  The phases follow, in the order the kernel calls them.
enum class KnnFilter {
    F32,     // Float32 GEMM
    F16,     // fp16 filter: every block centres, scales and converts its cloud (scale pass, producers convert while staging)
    F16Pre,  // fp16 filter on the pre-pass image (fx3d_knn_ws): x and y 16-byte aligned, D % 4 == 0 (knn_mfma_launch owns the condition)
};
template <int DK_, KnnFilter MODE>
struct KnnMfmaCfg {
    static constexpr int DK = DK_;
    static constexpr bool F16 = MODE != KnnFilter::F32, PRE = MODE == KnnFilter::F16Pre;
    static constexpr int DP = DK * 32;           // padded feature dimension
    static constexpr int RS = DP + 4;            // row stride of the query rows staged in the prologue (floats)
    static constexpr int PPR = DK * 8;           // 16-byte pieces per candidate row
    static constexpr int NT = DP / 8;            // b128 operand fetches per tile and half
    static constexpr int NB16 = DP / 16;         // K blocks of the fp16 filter
    static constexpr int RSI = F16 ? DP / 2 : DP;  // image row stride in floats (fp16: halves)
    static constexpr int PPI = RSI / 4;          // 16-byte pieces per image row
    static constexpr int RPB = PPI >= 16 ? 1 : 16 / PPI;  // fp16 image: rows per 256 bytes (knn_hpiece_off)
    // PRE: the image arrives without VALU work, so BOTH waves of a pair (they share a SIMD) run the filter, on alternate double
    // pairs of tiles: two waves per SIMD hide each other's LDS latencies and MFMA -> VALU dependencies (a lone consumer wave
    // stalled for more than half of its cycles).  Per query 128 group minima instead of 64 (a tighter tau), four lane lists
    // instead of two (the decode is shared by four lanes).
    static constexpr int LCAP = PRE ? kMLCap / 2 : kMLCap;  // rows of a lane's mask list
    // PRE, D <= 64: the next chunk of the image comes through REGISTERS -- every thread requests its 16-byte pieces before its
    // share of the filter and writes them to the other buffer after it (no VALU either way).  Direct-to-LDS loads move ~16 bytes
    // per cycle and CU and do not overlap the compute; loads to registers run at the L1's 64 bytes per cycle.  (D > 64: eight
    // pieces per thread -- 32 registers the kernel does not have; the producer waves' direct loads stay.)
    static constexpr bool REGST = PRE && DK <= 2;
    static constexpr int NCR = REGST ? (PPI / 2 > 0 ? PPI / 2 : 1) : 1;  // 16-byte pieces per thread and 256-row chunk
};

struct KnnMfmaArgs {
    const float *x;
    int N;
    const float *y;
    int M, B, D, k, drop;
    int32_t *idx;
    float *dist;
    int CH, img, keep_norms, two_norms, srl, csl;  // KnnMfmaPlan's fields (img: floats of the two chunk buffers)
    void *pre_ws;                                  // F16Pre: the pre-pass workspace
    int xdiv;                                      // > 1: candidate slices as virtual clouds share their queries
};

// The dynamic LDS of knn_mfma_kernel: the two chunk buffers (`img` floats: image [CH][RSI] + norms [CH] each; they also hold the
// scale pass's scratch, the staged query rows and, in the exact phase, the key arrays), then the regions below, as byte offsets
// from the end of the buffers.  Fixed-size bookkeeping first, then lists | med | norms: from the lists on everything is dead once
// the survivors are decoded, so the staged exact phase uses that whole tail of the allocation for candidate rows.
constexpr size_t kMListBytes = (size_t)kMWaves * kMLCap * 64 * 4;
constexpr size_t kMMedBytes = (size_t)2 * kMWaves * (kMMedCap + 128) * 4;
constexpr size_t kMSlotBytes = (size_t)kMWaves * 32 * 33 * 8;  // rank slots: [kMWaves][32][32 + 1 pad] keys
static_assert(kMSlotBytes + 2 * kMWaves * 128 * 4 <= kMListBytes, "rank slots + fallback scratch alias the mask lists");
struct KnnMfmaLds {
    size_t lcnt;    // [kMWaves][64] list lengths; PRE: [2 kMWaves][64] unsigned short in the same space
    size_t qn_n;    // [kMWaves][32] survivors per query
    size_t qflag;   // [kMWaves][32] 1 = fast path, 2 = medium path
    size_t qbelow;  // [kMWaves][32] entries with rank < kk
    size_t cmax;    // four words: bits of max |c|^2 (>= 0) | candidate-side error coefficient | skew flag | bulk radius
    size_t mu;      // [DP] fp16 filter without the pre-pass: per-dimension centre of the cloud
    size_t qstpk;   // [kMWaves][32] x 8 bytes: survivors per row stage (packed prefix)
    size_t lists;   // [kMWaves][kMLCap][64] mask words (PRE: [2 kMWaves][kMLCap / 2][64]); before them the tau exchange, after them
                    // the rank slots and (behind all the slots) the fallback scratch [2 kMWaves][128] words
    size_t med;     // [2 kMWaves][kMMedCap + 128] medium path: ids + merge lists
    size_t nall;    // [nchunk * CH] candidate norms, one array (keep_norms) or two (two_norms).  PRE: after the chunk loop the four
                    // parts' packed stage counts per query [kMWaves][32][4] x 8 bytes (4 KiB; the norm arrays are dead then and at
                    // least that large: one array of >= 2304 floats, or two of >= 512)
    static constexpr KnnMfmaLds make(int DP) {
        KnnMfmaLds l{};
        size_t o = 0;
        l.lcnt = o; o += (size_t)kMWaves * 64 * 4;
        l.qn_n = o; o += (size_t)kMWaves * 32 * 4;
        l.qflag = o; o += (size_t)kMWaves * 32 * 4;
        l.qbelow = o; o += (size_t)kMWaves * 32 * 4;
        l.cmax = o; o += 16;
        l.mu = o; o += (size_t)DP * 4;
        l.qstpk = o; o += (size_t)kMWaves * 32 * 8;
        l.lists = o; o += kMListBytes;
        l.med = o; o += kMMedBytes;
        l.nall = o;
        return l;
    }
    static constexpr size_t norm_bytes(int M) { return (size_t)((M + 255) / 256 * 256 + 256) * 4; }
    // 48 bytes that the plan has always counted with the bookkeeping and nothing uses: kept, so that CH, srl and the allocation
    // of every shape stay what they were
    static constexpr size_t kSlack = 48;
    constexpr size_t small() const { return lists + kSlack; }
    constexpr size_t bytes(int M, int norm_arrays) const { return nall + kSlack + norm_arrays * norm_bytes(M); }
};

// what every phase reads: the arguments, the block's LDS regions, the thread's coordinates
struct KnnMfmaCtx {
    KnnMfmaArgs a;
    float *sm;  // the chunk buffers
    int *lcnt, *qn_n, *qflag, *qbelow, *lists, *med;
    unsigned short *lcnt2;
    unsigned int *cmax;
    float *mu, *nall, *nallm;  // nallm: [nchunk * CH] norms for the phase-B test (two_norms), else nullptr
    unsigned long long *qstpk, *qpk;
    int buf_floats;  // one chunk buffer
    int b;           // cloud
    int tid, lane, wv, cw, ptid, half, h, jl, part;
    bool consumer, wave_active, vec4x, vec4y;
    int kk, q0, qi, nchunk;
    const float *xb, *yb;
    const _Float16 *pre_img;  // PRE: this cloud's image, norms and header in the workspace
    const float *pre_nup, *pre_ndn, *pre_hdr;
    const unsigned int *pre_cmax;
};

// ---- block and lane coordinates, LDS carve-up (arithmetic only: c.b >= B is a padding block, which the kernel leaves at once)
template <class T>
__device__ __forceinline__ void knn_mfma_coords(const KnnMfmaArgs &a, float *sm, KnnMfmaCtx &c) {
    constexpr KnnMfmaLds L = KnnMfmaLds::make(T::DP);
    c.a = a;
    c.sm = sm;
    c.buf_floats = a.CH * T::RSI + a.CH;
    unsigned char *fixed = reinterpret_cast<unsigned char *>(sm + a.img);
    c.lcnt = reinterpret_cast<int *>(fixed + L.lcnt);
    c.qn_n = reinterpret_cast<int *>(fixed + L.qn_n);
    c.qflag = reinterpret_cast<int *>(fixed + L.qflag);
    c.qbelow = reinterpret_cast<int *>(fixed + L.qbelow);
    c.cmax = reinterpret_cast<unsigned int *>(fixed + L.cmax);
    c.mu = reinterpret_cast<float *>(fixed + L.mu);
    c.qstpk = reinterpret_cast<unsigned long long *>(fixed + L.qstpk);
    c.lcnt2 = reinterpret_cast<unsigned short *>(fixed + L.lcnt);
    c.lists = reinterpret_cast<int *>(fixed + L.lists);
    c.med = reinterpret_cast<int *>(fixed + L.med);
    c.nall = reinterpret_cast<float *>(fixed + L.nall);
    c.qpk = reinterpret_cast<unsigned long long *>(fixed + L.nall);
    // block L runs on XCD L % 8: give every cloud's blocks ids with equal L % 8 so that its candidates stay in
    // one L2 (8 or more clouds; fewer: plain order, a cloud's blocks spread over all XCDs)
    const int nbx = (a.N + kMWaves * 32 - 1) / (kMWaves * 32);
    const int Lb = blockIdx.x;
    const bool by_xcd = a.B >= 8;
    c.b = by_xcd ? ((Lb >> 3) / nbx) * 8 + (Lb & 7) : Lb / nbx;
    const int bxq = by_xcd ? (Lb >> 3) % nbx : Lb % nbx;
    c.pre_img = nullptr;
    c.pre_nup = c.pre_ndn = c.pre_hdr = nullptr;
    c.pre_cmax = nullptr;
    if (T::PRE) {  // the workspace's layout is a function of (M, DP)
        const KnnPre pre = KnnPre::make(a.pre_ws, a.M, T::DP);
        c.pre_img = pre.img(c.b); c.pre_nup = pre.nup(c.b); c.pre_ndn = pre.ndn(c.b);
        c.pre_hdr = pre.hdr(c.b); c.pre_cmax = pre.cmaxp(c.b);
    }
    c.tid = threadIdx.x; c.lane = c.tid & 63; c.wv = c.tid >> 6;
    c.consumer = c.wv < kMWaves;
    c.cw = c.consumer ? c.wv : c.wv - kMWaves;   // the consumer wave this wave is paired with
    c.ptid = c.tid - kMProd;                     // producer thread id (negative for consumers)
    c.half = c.consumer ? 0 : 1;
    c.h = c.lane >> 5; c.jl = c.lane & 31;
    c.part = (c.consumer ? 0 : 2) + c.h;         // the query's four lanes: two half-waves x the pair's two waves
    c.kk = a.k + a.drop;
    c.xb = a.x + (size_t)(c.b / a.xdiv) * a.N * a.D;
    c.yb = a.y + (size_t)c.b * a.M * a.D;
    c.q0 = (bxq * kMWaves + c.cw) * 32;
    c.wave_active = c.q0 < a.N;
    c.qi = c.q0 + c.jl;
    c.vec4y = (a.D % 4 == 0) && ((reinterpret_cast<uintptr_t>(c.yb) & 15) == 0);
    c.vec4x = (a.D % 4 == 0) && ((reinterpret_cast<uintptr_t>(c.xb) & 15) == 0);
    c.nchunk = (a.M + a.CH - 1) / a.CH;
    c.nallm = a.two_norms ? c.nall + (size_t)c.nchunk * a.CH : nullptr;
}

// ---- scale.  sc: power-of-two scale with |sc * c| < 2^10 for every candidate; funit: unit of the absolute error terms (fp16
// filters; 1 and 1 for the Float32 GEMM).  cmax[0] is zero or the NaN pattern afterwards, cmax[1] the candidate-side coefficient.

// fp16 filter without the pre-pass, by every block: per-dimension MEAN mu (robust against a few far points, unlike the mid-range)
// and the largest |c - mu| of the cloud, one coalesced pass (F16 => 16-byte loads are legal).  Distances do not depend on the
// origin, the fp16 band does: it grows with |q~|^2 + |c~|^2, so a common offset of a few standard deviations would flood the
// lists.  Thread t always sees the same four dimensions when the block size is a multiple of D/4.  (Any mu is correct; it only
// has to be the same for all points.)
template <class T>
__device__ __forceinline__ void knn_mfma_scale_pass(const KnnMfmaCtx &c, float &sc, float &funit) {
    constexpr int DP = T::DP;
    const int tid = c.tid, lane = c.lane, wv = c.wv, D = c.a.D, M = c.a.M;
    const float *yb = c.yb;
    unsigned int *cmax = c.cmax;
    float *mu = c.mu;
    __syncthreads();
    const int rq = D / 4;
    const bool centre = (kMThreads % rq) == 0 && rq <= 32;
    float4 lo4 = float4{INFINITY, INFINITY, INFINITY, INFINITY}, hi4 = float4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    float4 sum4 = float4{0.f, 0.f, 0.f, 0.f};
    bool tnan = false;
    float poison = 0.0f;
    const float4 *c4 = reinterpret_cast<const float4 *>(yb);
    const int total4 = M * (D / 4);
    constexpr int kInFlight = 8;  // 16-byte loads in flight per thread (16 did not help: the pass is bound by the L2, every block reads its whole cloud)
    for (int e0 = tid; e0 < total4; e0 += kInFlight * kMThreads) {
        float4 v[kInFlight];
#pragma unroll
        for (int e = 0; e < kInFlight; ++e) v[e] = c4[e0 + e * kMThreads < total4 ? e0 + e * kMThreads : e0];  // (clamped: same dimensions)
#pragma unroll
        for (int e = 0; e < kInFlight; ++e) {
            // NaN or +-inf coordinates (x * 0 is NaN for them): no scale exists, every query takes the exact path
            poison = __builtin_fmaf(v[e].x, 0.0f, poison); poison = __builtin_fmaf(v[e].y, 0.0f, poison);
            poison = __builtin_fmaf(v[e].z, 0.0f, poison); poison = __builtin_fmaf(v[e].w, 0.0f, poison);
            lo4.x = vmin_f32(lo4.x, v[e].x); lo4.y = vmin_f32(lo4.y, v[e].y); lo4.z = vmin_f32(lo4.z, v[e].z); lo4.w = vmin_f32(lo4.w, v[e].w);
            hi4.x = vmax_f32(hi4.x, v[e].x); hi4.y = vmax_f32(hi4.y, v[e].y); hi4.z = vmax_f32(hi4.z, v[e].z); hi4.w = vmax_f32(hi4.w, v[e].w);
            if (e0 + e * kMThreads < total4) {  // (the clamped duplicates must not enter the mean)
                sum4.x = sum4.x + v[e].x; sum4.y = sum4.y + v[e].y; sum4.z = sum4.z + v[e].z; sum4.w = sum4.w + v[e].w;
            }
        }
    }
    tnan = poison != poison;
    const bool anynan = __syncthreads_or(tnan) != 0;
    float *red = c.sm;  // [kMThreads / 64][32][12] scratch in the (still unused) chunk buffers
    if (centre) {
        for (int m = rq; m < 64; m <<= 1) {  // lanes with equal lane % rq hold the same dimensions
            lo4.x = fminf(lo4.x, __shfl_xor(lo4.x, m, 64)); lo4.y = fminf(lo4.y, __shfl_xor(lo4.y, m, 64));
            lo4.z = fminf(lo4.z, __shfl_xor(lo4.z, m, 64)); lo4.w = fminf(lo4.w, __shfl_xor(lo4.w, m, 64));
            hi4.x = fmaxf(hi4.x, __shfl_xor(hi4.x, m, 64)); hi4.y = fmaxf(hi4.y, __shfl_xor(hi4.y, m, 64));
            hi4.z = fmaxf(hi4.z, __shfl_xor(hi4.z, m, 64)); hi4.w = fmaxf(hi4.w, __shfl_xor(hi4.w, m, 64));
            sum4.x = sum4.x + __shfl_xor(sum4.x, m, 64); sum4.y = sum4.y + __shfl_xor(sum4.y, m, 64);
            sum4.z = sum4.z + __shfl_xor(sum4.z, m, 64); sum4.w = sum4.w + __shfl_xor(sum4.w, m, 64);
        }
        if (lane < rq) {
            float *r8 = red + (size_t)(wv * 32 + lane) * 12;
            r8[0] = lo4.x; r8[1] = lo4.y; r8[2] = lo4.z; r8[3] = lo4.w;
            r8[4] = hi4.x; r8[5] = hi4.y; r8[6] = hi4.z; r8[7] = hi4.w;
            r8[8] = sum4.x; r8[9] = sum4.y; r8[10] = sum4.z; r8[11] = sum4.w;
        }
    }
    __syncthreads();
    float amax = 0.0f;
    if (centre) {
        if (tid < rq) {
            float lo[4] = {INFINITY, INFINITY, INFINITY, INFINITY}, hi[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            float sm4[4] = {0.f, 0.f, 0.f, 0.f};
            for (int w = 0; w < kMThreads / 64; ++w) {
                const float *r8 = red + (size_t)(w * 32 + tid) * 12;
#pragma unroll
                for (int e = 0; e < 4; ++e) { lo[e] = fminf(lo[e], r8[e]); hi[e] = fmaxf(hi[e], r8[4 + e]); sm4[e] = sm4[e] + r8[8 + e]; }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float m0 = sm4[e] / (float)M;
                m0 = fminf(fmaxf(m0, lo[e]), hi[e]);  // (rounding of the sum cannot leave the range)
                mu[4 * tid + e] = m0;
                amax = fmaxf(amax, fmaxf(hi[e] - m0, m0 - lo[e]));
                // a mean far from the middle of its range: skewed data or a few far points (checked below on a sample)
                if (fabsf(m0 - 0.5f * (lo[e] + hi[e])) > 0.25f * (hi[e] - lo[e])) cmax[2] = 1u;
            }
        } else if (tid < DP / 4) {
            mu[4 * tid] = 0.0f; mu[4 * tid + 1] = 0.0f; mu[4 * tid + 2] = 0.0f; mu[4 * tid + 3] = 0.0f;
        }
    } else {
        if (tid < DP / 4) { mu[4 * tid] = 0.0f; mu[4 * tid + 1] = 0.0f; mu[4 * tid + 2] = 0.0f; mu[4 * tid + 3] = 0.0f; }
        if (tid < total4)  // (threads without an element hold +-inf)
            amax = fmaxf(fmaxf(fmaxf(fabsf(lo4.x), fabsf(hi4.x)), fmaxf(fabsf(lo4.y), fabsf(hi4.y))),
                         fmaxf(fmaxf(fabsf(lo4.z), fabsf(hi4.z)), fmaxf(fabsf(lo4.w), fabsf(hi4.w))));
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) amax = fmaxf(amax, __shfl_xor(amax, m, 64));
    if (lane == 0) atomicMax(cmax, anynan ? 0x7fc00000u : __builtin_bit_cast(unsigned int, amax));
    __syncthreads();
    if (centre && cmax[2] != 0u && !anynan) {  // (block-uniform)
        // ---- robust centre.  A few points far from the bulk pull the mean towards them (one point 10^6 x the extent away
        //      among 1024: by 10^3 extents), every query then sits |q~| >> extent from the centre and its band ~ 2^-10 |q~|^2
        //      swallows the whole cloud (1.7 ms instead of 80 us).  Per-dimension MEDIAN and quartiles of 16 rows spread
        //      over the cloud; when a mean lies more than 8 interquartile ranges from the median, every dimension is
        //      centred on its median instead (any centre is correct) and the extent grows by the largest shift (an upper
        //      bound, no second pass).  Skewed but clean data (one-sided features) keep their means.
        if (wv == 0) {
            float shiftmax = 0.0f, iqr2 = 0.0f;
            bool sw = false;
            float medv[DP / 64 > 0 ? DP / 64 : 1];
#pragma unroll
            for (int t = 0; t < (DP + 63) / 64; ++t) {
                const int d = lane + 64 * t;
                float v[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) v[i] = yb[(size_t)((long long)i * M / 16) * D + (d < D ? d : 0)];
                float med = v[0], q1 = v[0], q3 = v[0];
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    int rk = 0;
#pragma unroll
                    for (int j = 0; j < 16; ++j) rk += (v[j] < v[i] || (v[j] == v[i] && j < i)) ? 1 : 0;
                    med = rk == 8 ? v[i] : med; q1 = rk == 4 ? v[i] : q1; q3 = rk == 12 ? v[i] : q3;
                }
                const float shift = d < D ? fabsf(mu[d < D ? d : 0] - med) : 0.0f;
                sw = sw || (shift > 8.0f * (q3 - q1));
                shiftmax = fmaxf(shiftmax, shift);
                if (d < D) iqr2 = __builtin_fmaf(q3 - q1, q3 - q1, iqr2);
                medv[t] = med;
            }
            if (__ballot(sw) != 0ull) {
#pragma unroll
                for (int m = 1; m < 64; m <<= 1) {
                    shiftmax = fmaxf(shiftmax, __shfl_xor(shiftmax, m, 64));
                    iqr2 = iqr2 + __shfl_xor(iqr2, m, 64);
                }
#pragma unroll
                for (int t = 0; t < (DP + 63) / 64; ++t)
                    if (lane + 64 * t < D) mu[lane + 64 * t] = medv[t];
                if (lane == 0) {
                    *cmax = __builtin_bit_cast(unsigned int, __builtin_bit_cast(float, *cmax) + shiftmax);
                    reinterpret_cast<float *>(cmax)[3] = sqrtf(iqr2);  // the bulk's radius (unscaled): the unit of the absolute error terms below
                }
            }
        }
        __syncthreads();
    }
    const float cinf = __builtin_bit_cast(float, *cmax);
    if (cinf > kTinyExtent && cinf < 1.0e30f) {
        int e;
        (void)frexpf(cinf * 1.000001f, &e);  // = m 2^e, m in [0.5, 1)
        // |sc (c - mu)| < 2^10: ten binades above 1 so that a bulk far smaller than the largest |c - mu| (a few far
        // points) still sits in fp16's normal range; queries up to 30 x the cloud's extent stay below 6e4
        sc = ldexpf(1.0f, 10 - e);
    }
    {
        // unit s of the absolute (fp16 subnormal) error terms: |x| <= (x^2 / s + s) / 2 for any s > 0 turns the linear bound
        // 2^-24 sqrt(D) (|q~| + |c~| / 2) into shares of the squared norms.  s = 1 unless the cloud was centred on its medians
        // because of far points: then the bulk may sit far below 1 in scaled units, and with s = 1 the constant term
        // 2^-23 sqrt(D) would dwarf its squared distances (the whole cloud inside every band).
        const float rad = reinterpret_cast<const float *>(cmax)[3];
        funit = rad > 0.0f ? fminf(1.0f, fmaxf(sc * rad, 0x1p-12f)) : 1.0f;
    }
    __syncthreads();
    if (tid == 0 && funit < 1.0f) {
        const float aq = 8.0f * (float)(4 * D + 8) * 0x1p-24f + 0x1.01p-10f;
        reinterpret_cast<float *>(cmax)[1] = aq * 1.01f + 0x1p-26f * sqrtf((float)D) / funit + 0x1p-23f;
    }
    // from here on: bits of the largest SCALED squared norm.  A cloud whose extent lets exact Float32 distances overflow
    // (D (61 cinf)^2 >= 3.4e38 for usable queries) is handled like a non-finite one: its +Inf ties are ordered by index in
    // the oracle, which only the brute-force merge reproduces.
    if (tid == 0) *cmax = (anynan || !(cinf < 1.0e15f)) ? 0x7fc00000u : 0u;
}

// behind the pre-pass: its header has the centre, the scale and the largest scaled norm of this cloud.  No barrier: thread 0
// alone wrote the words it overwrites, and they are read after the chunk loop's barriers.
__device__ __forceinline__ void knn_mfma_read_header(const KnnMfmaCtx &c, float &sc, float &funit) {
    const float *h = c.pre_hdr;
    sc = h[0];
    funit = h[1];
    if (c.tid == 0) {
        reinterpret_cast<float *>(c.cmax)[1] = h[2];
        unsigned int m = h[3] != 0.0f ? 0x7fc00000u : 0u;
        const unsigned int *cp = c.pre_cmax;
        for (int p = 0; p < kPreParts; ++p) m = cp[p] > m ? cp[p] : m;  // (NaN pattern > every finite norm)
        *c.cmax = m;
    }
}

template <class T>
__device__ __forceinline__ void knn_mfma_scale(const KnnMfmaCtx &c, float &sc, float &funit) {
    if (c.tid == 0) {
        unsigned int *cmax = c.cmax;
        const int D = c.a.D;
        *cmax = 0u;
        cmax[2] = 0u;  // F16: a mean far from the middle of its range was seen (scale pass)
        cmax[3] = 0u;  // F16: bulk radius of a cloud centred on its medians (0: not in use)
        // filter error per unit of (candidate norm + query norm), scaled units: fp32 accumulation + centring + the oracle's own
        // rounding 8 (4D + 8) u (4x head-room), operand representation 2^-10 (rounded halves; the Float32 GEMM, which
        // never reads it, parks 2^-18)
        const float aq = 8.0f * (float)(4 * D + 8) * 0x1p-24f + (T::F16 ? 0x1.01p-10f : 0x1p-18f);
        // candidate side: + its share of the subnormal floor, + the rounding of n (1 +- A); parked in LDS (cmax[1])
        reinterpret_cast<float *>(cmax)[1] = aq * 1.01f + 0x1p-26f * sqrtf((float)D) + 0x1p-23f;
    }
    sc = 1.0f;
    funit = 1.0f;
    if (T::PRE) knn_mfma_read_header(c, sc, funit);
    else if (T::F16) knn_mfma_scale_pass<T>(c, sc, funit);
}

// ---- query operand: the B operand of the filter, the wave's 32 query rows as -2 q in registers
template <class T>
struct KnnQueryOp {
    float4 a[T::NT];     // f32 filter: -2 q, this lane's half of the permuted reduction dimension
    kh8 ah[T::NB16];     // fp16 filter: halves of -2 sc (q - mu), 8 dimensions per K block and half-wave
    float qn;            // |q|^2 (fp16: of the centred, scaled row)
    bool qok;            // fp16: the operand is inside the fp16 range
};
// eight centred and scaled query values -> their halves of -2 q~, the norm and the largest operand
__device__ __forceinline__ kh8 knn_query_halves(const float (&qs)[8], float &qn, float &amax) {
    kh8 r;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        qn = qn + qs[e] * qs[e];
        const float av = -2.0f * qs[e];
        amax = fmaxf(amax, fabsf(av));
        r[e] = (_Float16)av;
    }
    return r;
}
// PRE: every lane reads its pieces of its query row and of the centre straight from memory, all loads in flight together: with
// the first chunk requested behind them (knn_mfma_first_chunk_request) the kernel's start is ONE global round trip -- no staging
// of the query rows through LDS, no barrier before the first chunk's.  K block bb covers dimensions 16 bb + 8 h + [0, 8) in
// half-wave h (16 bytes of the lane's own row -- rows beyond N read row N - 1 and are never used -- and of the pre-pass
// header's centre, zero beyond D).
template <class T>
__device__ __forceinline__ void knn_mfma_query_load(const KnnMfmaCtx &c, float4 (&qv)[T::NB16][2], float4 (&mv)[T::NB16][2]) {
    const int D = c.a.D, N = c.a.N;
    const float *qg = c.xb + (size_t)(c.qi < N ? c.qi : N - 1) * D;
    const float *mg = c.pre_hdr + 8;
#pragma unroll
    for (int bb = 0; bb < T::NB16; ++bb)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int d0 = 16 * bb + 8 * c.h + 4 * u;
            qv[bb][u] = *reinterpret_cast<const float4 *>(qg + (d0 < D ? d0 : 0));
            mv[bb][u] = *reinterpret_cast<const float4 *>(mg + d0);
        }
}
template <class T>
__device__ __forceinline__ void knn_mfma_query_operand_pre(const KnnMfmaCtx &c, const float4 (&qv)[T::NB16][2], const float4 (&mv)[T::NB16][2],
                                                           float sc, KnnQueryOp<T> &q) {
    float amax = 0.0f;
#pragma unroll
    for (int bb = 0; bb < T::NB16; ++bb) {
        float qs[8];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const bool in = 16 * bb + 8 * c.h + 4 * u < c.a.D;
            const float v[4] = {qv[bb][u].x, qv[bb][u].y, qv[bb][u].z, qv[bb][u].w}, m4[4] = {mv[bb][u].x, mv[bb][u].y, mv[bb][u].z, mv[bb][u].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) qs[4 * u + e] = in ? (v[e] - m4[e]) * sc : 0.0f;  // centred like the candidates
        }
        q.ah[bb] = knn_query_halves(qs, q.qn, amax);
    }
    amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
    q.qok = amax < 6.0e4f;  // inside the fp16 range (false for NaN too)
    q.qn = q.qn + __shfl_xor(q.qn, 32, 64);
}
// without the pre-pass: the consumer waves stage their query rows through LDS (coalesced; x may be unaligned, D any)
template <class T>
__device__ __forceinline__ void knn_mfma_query_operand_lds(const KnnMfmaCtx &c, float sc, KnnQueryOp<T> &q) {
    constexpr int DP = T::DP, RS = T::RS;
    const int D = c.a.D, N = c.a.N, lane = c.lane, h = c.h, jl = c.jl;
    if (c.consumer) {
        float *qs = c.sm + (size_t)c.cw * 32 * RS;
        const int nrow = c.wave_active ? ((N - c.q0) < 32 ? (N - c.q0) : 32) : 0;
        const float *src = c.xb + (size_t)c.q0 * D;
        if (c.vec4x) {
            const int rq = D / 4;
            for (int e = lane; e < nrow * rq; e += 64) {
                const int row = e / rq, c4 = e - row * rq;
                *reinterpret_cast<float4 *>(qs + (size_t)row * RS + 4 * c4) = reinterpret_cast<const float4 *>(src)[e];
            }
        } else {
            for (int e = lane; e < nrow * D; e += 64) {
                const int row = e / D, d = e - row * D;
                qs[(size_t)row * RS + d] = src[e];
            }
        }
        for (int e = lane; e < 32 * DP; e += 64) {  // zero padding: columns >= D, rows >= nrow
            const int row = e / DP, d = e - row * DP;
            if (row >= nrow || d >= D) qs[(size_t)row * RS + d] = 0.0f;
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
        if (T::F16) {
            // K block bb covers dimensions 16 bb + 8 h + [0, 8) in half-wave h
            float amax = 0.0f;
#pragma unroll
            for (int bb = 0; bb < T::NB16; ++bb) {
                const float *qr = qs + (size_t)jl * RS + 16 * bb + 8 * h;
                const float4 v0 = *reinterpret_cast<const float4 *>(qr), v1 = *reinterpret_cast<const float4 *>(qr + 4);
                const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
                float qsc[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) qsc[e] = (v[e] - c.mu[16 * bb + 8 * h + e]) * sc;  // centred like the candidates
                q.ah[bb] = knn_query_halves(qsc, q.qn, amax);
            }
            amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
            q.qok = amax < 6.0e4f;  // inside the fp16 range (false for NaN too)
        } else {
            const float *qr = qs + (size_t)jl * RS + h * (DP / 2);
#pragma unroll
            for (int t = 0; t < T::NT; ++t) {
                const float4 v = *reinterpret_cast<const float4 *>(qr + 4 * t);
                q.qn = q.qn + v.x * v.x;
                q.qn = q.qn + v.y * v.y;
                q.qn = q.qn + v.z * v.z;
                q.qn = q.qn + v.w * v.w;
                q.a[t] = float4{-2.0f * v.x, -2.0f * v.y, -2.0f * v.z, -2.0f * v.w};
            }
        }
        q.qn = q.qn + __shfl_xor(q.qn, 32, 64);
    }
    __syncthreads();
}

// ---- first chunk
// fp16 filter without the pre-pass: what the producers carry from one staging event to the next
struct KnnProducer {
    float4 preg[kMUnits][2];  // the chunk after next, loaded one step ahead
    float pmax;               // largest scaled norm seen
    bool pnan;
    int stage_ev;             // staging events done (chunks 0..n-1, n-2..0)
};
__device__ __forceinline__ void knn_publish_pmax(const KnnMfmaCtx &c, KnnProducer &p) {  // this wave's maximum norm
    float pmax = p.pmax;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) pmax = fmaxf(pmax, __shfl_xor(pmax, m, 64));
    p.pmax = pmax;
    const bool anyn = __ballot(p.pnan) != 0;
    if (c.lane == 0) atomicMax(c.cmax, anyn ? 0x7fc00000u : __builtin_bit_cast(unsigned int, pmax));
}
// PRE: the producers request the first chunk of the image and, D <= 64 (the image chunks of the loop come through registers),
// the norms of ALL chunks, once.  Called BEHIND the wave's own query loads: the memory counter retires in order, so requested
// first they made the producer waves wait for the whole chunk before they could touch their header values.
template <class T>
__device__ __forceinline__ void knn_mfma_first_chunk_request(const KnnMfmaCtx &c) {
    const int CH = c.a.CH;
    if (!c.consumer) {
        if (T::REGST)
            for (int ch = 1; ch < c.nchunk; ++ch)
                knn_pre_stage_norms(c.pre_nup, c.pre_ndn, ch * CH, CH, c.nall + (size_t)ch * CH, c.nallm ? c.nallm + (size_t)ch * CH : nullptr,
                                    c.wv - kMWaves, c.lane);
        knn_pre_stage_chunk<T::DK>(c.pre_img, c.pre_nup, c.pre_ndn, 0, CH, c.sm, c.nall, c.nallm, true, c.wv - kMWaves, c.lane);
    }
}
// the first chunk is resident in buffer 0 behind this function's barrier
template <class T>
__device__ __forceinline__ void knn_mfma_first_chunk(const KnnMfmaCtx &c, float sc, KnnProducer &p) {
    constexpr int DK = T::DK, DP = T::DP;
    const int M = c.a.M, D = c.a.D, CH = c.a.CH;
    p.pmax = 0.0f;
    p.pnan = false;
    p.stage_ev = 0;
    const int nevents = 2 * c.nchunk - 1;
    if (T::PRE) {
        if (!c.consumer) {
            __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0): this wave's pieces of the first chunk (requested at the kernel's start) have landed
            __builtin_amdgcn_wave_barrier();
        }
    } else if (T::F16) {
        if (!c.consumer) {
            knn_f16_load_chunk<DK>(c.yb, D, 0, M < CH ? M : CH, CH, c.ptid, p.preg);
            knn_f16_store_chunk<DK>(c.sm, CH, M < CH ? M : CH, sc, c.mu, c.ptid, p.preg, c.nall, c.nallm, reinterpret_cast<const float *>(c.cmax + 1), p.pmax, p.pnan);
            if (c.nchunk == 1) knn_publish_pmax(c, p);
            if (nevents > 1) {
                const int c1 = 1 < c.nchunk ? 1 : 2 * c.nchunk - 3;
                knn_f16_load_chunk<DK>(c.yb, D, c1 * CH, (M - c1 * CH) < CH ? (M - c1 * CH) : CH, CH, c.ptid, p.preg);
            }
            p.stage_ev = 1;
        }
    } else {
        if (D < DP || !c.vec4y) {  // padding columns must read as zeros; the direct loads never touch them
            for (int e = c.tid; e < 2 * c.buf_floats / 4; e += kMThreads)
                reinterpret_cast<float4 *>(c.sm)[e] = float4{0.f, 0.f, 0.f, 0.f};
            __syncthreads();
        }
        if (!c.consumer) {
            const int cn = M < CH ? M : CH;
            knn_stage_chunk<DK>(c.yb, D, 0, cn, CH, c.sm, c.a.keep_norms ? c.nall : c.sm + (size_t)CH * DP, c.cmax, true, true, c.vec4y,
                                c.wv - kMWaves, c.lane);
        }
    }
    __syncthreads();
}

// ---- chunk loop.  Phase A walks the chunks forwards (group minima), phase B backwards (its first chunk is resident; mask lists)
struct KnnStep {
    int phase, ci, j0, cn_pad;  // this step's chunk
    int nstep1, ci_next;        // the next step and its chunk
    bool stage_next;            // the next step needs another chunk than this one
};
__device__ __forceinline__ KnnStep knn_mfma_step(const KnnMfmaCtx &c, int step) {
    KnnStep s;
    const int nstep = 2 * c.nchunk, M = c.a.M, CH = c.a.CH;
    s.phase = step >= c.nchunk ? 1 : 0;
    s.ci = s.phase ? nstep - 1 - step : step;
    s.j0 = s.ci * CH;
    const int cn = (M - s.j0) < CH ? (M - s.j0) : CH;
    s.cn_pad = (cn + 63) & ~63;
    s.nstep1 = step + 1;
    s.ci_next = s.nstep1 >= c.nchunk ? nstep - 1 - s.nstep1 : s.nstep1;
    s.stage_next = s.nstep1 < nstep && s.ci_next != s.ci;
    return s;
}
// what the filter leaves per lane
struct KnnFilterOut {
    float mn[32];  // group minima: [r] even tiles, [16 + r] odd tiles -> 64 groups per query (PRE: 128, with the pair's other wave)
    float thr;     // phase B's threshold
    int cnt;       // list words with a survivor
    int totb;      // survivors seen by phase B (all of them: the overflow flag tells when words were lost)
    int *mylist;   // entry e at mylist[e * 64]
};
// one word per tile: (tile index << 16) | mask of the rows with F <= thr; stored at the list head unconditionally, the head
// advances when the mask is not empty
template <class T>
__device__ __forceinline__ void knn_list_push(KnnFilterOut &f, int tile, unsigned int m) {
    const int pp = f.cnt < T::LCAP - 1 ? f.cnt : T::LCAP - 1;
    f.mylist[pp * 64] = (int)((unsigned int)tile << 16 | m);
    f.cnt += m != 0 ? 1 : 0;
    f.totb += __builtin_popcount(m);
}
// PRE: TWO pairs of tiles per iteration -- the second pair's operand fetches and MFMAs are issued before the first pair's
// results are folded, so the fold (VALU) of one overlaps the matrix work of the other and one round of LDS latency serves four
// tiles.  (Without the pre-pass the producers' staging registers leave no room: 68 spills.)  One instantiation per phase: phase
// A's accumulators ARE the norm loads' destinations (no VALU) and two tiles fold per v_min3 straight from the MFMA registers;
// phase B starts them at n_c - thr (one v_sub each).  Returns the first pair it left.
template <class T, bool PHB>
__device__ __forceinline__ int knn_filter_quads(const KnnMfmaCtx &c, const KnnQueryOp<T> &qo, KnnFilterOut &f, const float *cand,
                                                const float *cnorm, int npair, int tile0) {
    constexpr int NB16 = T::NB16, RSI = T::RSI, PPI = T::PPI;
    const int h = c.h, jl = c.jl;
    const float thr = f.thr;
    int pr_first = 0;
    for (; pr_first + 1 < npair; pr_first += 2) {
        if (((pr_first >> 1) & 1) != c.half) continue;  // the pair's waves take alternate double pairs
        f32x16v accs[4];
        kh8 ops[4][NB16];
#pragma unroll
        for (int q = 0; q < 4; ++q) {  // q = 2 * (pair) + (tile of the pair)
            const int rbase = (pr_first + (q >> 1)) * 64 + 32 * (q & 1);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 n0 = *reinterpret_cast<const float4 *>(cnorm + rbase + 8 * g + 4 * h);
                if (PHB) {
                    accs[q][4 * g] = n0.x - thr; accs[q][4 * g + 1] = n0.y - thr; accs[q][4 * g + 2] = n0.z - thr; accs[q][4 * g + 3] = n0.w - thr;
                } else {
                    accs[q][4 * g] = n0.x; accs[q][4 * g + 1] = n0.y; accs[q][4 * g + 2] = n0.z; accs[q][4 * g + 3] = n0.w;
                }
            }
            const float *cq = cand + (size_t)(rbase + jl) * RSI;
#pragma unroll
            for (int bb = 0; bb < NB16; ++bb)
                ops[q][bb] = *reinterpret_cast<const kh8 *>(cq + ((2 * bb + h + jl / T::RPB) & (PPI - 1)) * 4);
        }
#pragma unroll
        for (int bb = 0; bb < NB16; ++bb) {  // four independent accumulators in turn: no MFMA waits for its predecessor
#pragma unroll
            for (int q = 0; q < 4; ++q) accs[q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ops[q][bb], qo.ah[bb], accs[q], 0, 0, 0);
        }
        // the fold / mask work runs at raised wave priority: the pair's other wave is then the one whose MFMAs are in the pipe
        // while this one issues VALU (the reverse, priority on the MFMA block, lets the issuing wave hog the slots its partner's
        // fold needs; static priorities by wave role have no effect)
        __builtin_amdgcn_s_setprio(1);
        if (!PHB) {
            // (any partition of the tiles into the 32 groups of a lane will do; the two accumulators issued last are
            //  read 20+ issue slots after their MFMAs: knn_f16_d3_kernel's order)
            KNN_MFMA_SETTLE4(accs[0], accs[1], accs[2], accs[3]);
#pragma unroll
            for (int r = 0; r < 16; ++r) asm volatile("v_min3_f32 %0, %0, %1, %2" : "+v"(f.mn[r]) : "v"(accs[0][r]), "v"(accs[1][r]));
#pragma unroll
            for (int r = 0; r < 16; ++r) asm volatile("v_min3_f32 %0, %0, %1, %2" : "+v"(f.mn[16 + r]) : "v"(accs[2][r]), "v"(accs[3][r]));
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                unsigned int m = 0;
#pragma unroll
                for (int i = 0; i < 16; ++i) {  // the sign of F - thr is the test: one v_alignbit per row shifts it in (row r at bit r)
                    const float av = accs[q][15 - i];
                    m = __builtin_amdgcn_alignbit(m, __builtin_bit_cast(unsigned int, av), 31);
                }
                knn_list_push<T>(f, tile0 + pr_first * 2 + q, m);
            }
        }
        __builtin_amdgcn_s_setprio(0);
    }
    return pr_first;
}
// one pair of tiles per iteration, pairs [pr_first, npair): every mode (PRE: a last lone pair)
template <class T>
__device__ __forceinline__ void knn_filter_pairs(const KnnMfmaCtx &c, const KnnQueryOp<T> &qo, KnnFilterOut &f, const float *cand,
                                                 const float *cnorm, int phase, int pr_first, int npair, int tile0) {
    constexpr int NB16 = T::NB16, RSI = T::RSI, PPI = T::PPI, NT = T::NT, PPR = T::PPR;
    constexpr bool F16 = T::F16;
    const int h = c.h, jl = c.jl;
    const float thr = f.thr;
    // phase B of the fp16 filters accumulates on n_c - thr: the sign of the result is the test.  (The Float32 GEMM keeps the
    // compare: its staging leaves the rows beyond the cloud's end unwritten -- norm +inf, stale pieces -- and inf + NaN has
    // no usable sign; the fp16 images are zero there.)
    const float tsub = (F16 && phase) ? thr : 0.0f;
    for (int pr = pr_first; pr < npair; ++pr) {
        // rows pr*64 + jl and + 32 share (row mod PPR) = jl mod PPR: one rotated offset per fetch
        const float *c0 = cand + (size_t)(pr * 64 + jl) * RSI, *c1 = c0 + (size_t)32 * RSI;
        // accumulators start at the candidate norms: register r of half h is row (r&3) + 8(r>>2) + 4h
        f32x16v acc0, acc1;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 n0 = *reinterpret_cast<const float4 *>(cnorm + pr * 64 + 8 * g + 4 * h);
            const float4 n1 = *reinterpret_cast<const float4 *>(cnorm + pr * 64 + 32 + 8 * g + 4 * h);
            acc0[4 * g] = n0.x - tsub; acc0[4 * g + 1] = n0.y - tsub; acc0[4 * g + 2] = n0.z - tsub; acc0[4 * g + 3] = n0.w - tsub;
            acc1[4 * g] = n1.x - tsub; acc1[4 * g + 1] = n1.y - tsub; acc1[4 * g + 2] = n1.z - tsub; acc1[4 * g + 3] = n1.w - tsub;
        }
        if (F16) {
            // one MFMA per K block and tile on the rounded halves
            kh8 h0[NB16], h1[NB16];
#pragma unroll
            for (int bb = 0; bb < NB16; ++bb) {
                const int ph = ((2 * bb + h + jl / T::RPB) & (PPI - 1)) * 4;
                h0[bb] = *reinterpret_cast<const kh8 *>(c0 + ph);
                h1[bb] = *reinterpret_cast<const kh8 *>(c1 + ph);
            }
#pragma unroll
            for (int bb = 0; bb < NB16; ++bb) {
                acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(h0[bb], qo.ah[bb], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(h1[bb], qo.ah[bb], acc1, 0, 0, 0);
            }
        } else {
            float4 b0[NT], b1[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int po = ((h * NT + t + jl) & (PPR - 1)) * 4;
                b0[t] = *reinterpret_cast<const float4 *>(c0 + po);
                b1[t] = *reinterpret_cast<const float4 *>(c1 + po);
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) {  // A = candidates (rows), B = queries (columns)
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(b0[t].x, qo.a[t].x, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(b1[t].x, qo.a[t].x, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(b0[t].y, qo.a[t].y, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(b1[t].y, qo.a[t].y, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(b0[t].z, qo.a[t].z, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(b1[t].z, qo.a[t].z, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(b0[t].w, qo.a[t].w, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(b1[t].w, qo.a[t].w, acc1, 0, 0, 0);
            }
        }
        if (phase == 0) {
            KNN_MFMA_SETTLE2(acc0, acc1);
#pragma unroll
            for (int r = 0; r < 16; ++r) f.mn[r] = vmin_acc(f.mn[r], acc0[r]);
#pragma unroll
            for (int r = 0; r < 16; ++r) f.mn[16 + r] = vmin_acc(f.mn[16 + r], acc1[r]);
        } else {
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                unsigned int m = 0;
#pragma unroll
                for (int i = 0; i < 16; ++i) {  // (ascending i: a descending unrolled loop over the vector's elements read element 0 every time)
                    const float av = tt ? acc1[15 - i] : acc0[15 - i];
                    if (F16) m = __builtin_amdgcn_alignbit(m, __builtin_bit_cast(unsigned int, av), 31);
                    else m |= (av <= thr) ? (1u << (15 - i)) : 0u;
                }
                knn_list_push<T>(f, tile0 + pr * 2 + tt, m);
            }
        }
    }
}
// the filter of one step: this wave's tiles of the chunk in buffer `cur`
template <class T>
__device__ __forceinline__ void knn_mfma_filter(const KnnMfmaCtx &c, const KnnStep &s, int cur, const KnnQueryOp<T> &qo, KnnFilterOut &f) {
    const int CH = c.a.CH;
    const float *cand = c.sm + (size_t)cur * c.buf_floats;
    const float *cnorm = c.a.keep_norms ? (s.phase && c.nallm ? c.nallm : c.nall) + (size_t)s.ci * CH : cand + (size_t)CH * T::DP;
    const int npair = s.cn_pad / 64;
    const int tile0 = s.j0 / 32;
    int pr_first = 0;
    if (T::PRE) {
        if (s.phase == 0) pr_first = knn_filter_quads<T, false>(c, qo, f, cand, cnorm, npair, tile0);
        else pr_first = knn_filter_quads<T, true>(c, qo, f, cand, cnorm, npair, tile0);
        if (c.half) pr_first = npair;  // a last lone pair goes to the first wave
    }
    knn_filter_pairs<T>(c, qo, f, cand, cnorm, s.phase, pr_first, npair, tile0);
}
// PRE staging of the next chunk, in two halves around the filter: the requests first (they land while this wave computes) ...
template <class T>
__device__ __forceinline__ void knn_mfma_stage_request_pre(const KnnMfmaCtx &c, const KnnStep &s, int cur, f32x4v (&creg)[T::NCR]) {
    constexpr int PPI = T::PPI;
    const int CH = c.a.CH, j0n = s.ci_next * CH;
    if (T::REGST) {
#pragma unroll
        for (int i = 0; i < T::NCR; ++i) {
            const int S = c.tid + i * kMThreads;
            const int row = S / PPI, pos = S & (PPI - 1);
            const int cc = (pos - row / T::RPB) & (PPI - 1);
            if (S < CH * PPI) creg[i] = *reinterpret_cast<const f32x4v *>(c.pre_img + ((size_t)(j0n + row) * PPI + cc) * 8);
        }
    } else if (!c.consumer) {  // (phase B brings the image only: the norms of all chunks stay in LDS)
        knn_pre_stage_chunk<T::DK>(c.pre_img, c.pre_nup, c.pre_ndn, j0n, CH, c.sm + (size_t)(1 - cur) * c.buf_floats,
                                          c.nall + (size_t)s.ci_next * CH, c.nallm ? c.nallm + (size_t)s.ci_next * CH : nullptr,
                                          s.nstep1 < c.nchunk, c.wv - kMWaves, c.lane);
    }
}
// ... and behind it the stores of the pieces held in registers, or the wait for the direct loads
template <class T>
__device__ __forceinline__ void knn_mfma_stage_finish_pre(const KnnMfmaCtx &c, int cur, const f32x4v (&creg)[T::NCR]) {
    if (T::REGST) {
        float *nimg = c.sm + (size_t)(1 - cur) * c.buf_floats;
#pragma unroll
        for (int i = 0; i < T::NCR; ++i) {
            const int S = c.tid + i * kMThreads;
            if (S < c.a.CH * T::PPI) *reinterpret_cast<f32x4v *>(nimg + (size_t)S * 4) = creg[i];
        }
    } else if (!c.consumer) {
        __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0): this wave's pieces of the next chunk have landed
        __builtin_amdgcn_wave_barrier();
    }
}
// fp16 filter without the pre-pass, producers: the registers hold chunk ci_next (loaded one step ago); convert and store it, then
// fetch the chunk after it
template <class T>
__device__ __forceinline__ void knn_mfma_stage_next_f16(const KnnMfmaCtx &c, const KnnStep &s, int cur, float sc, KnnProducer &p) {
    const int M = c.a.M, CH = c.a.CH, nchunk = c.nchunk, nevents = 2 * c.nchunk - 1;
    const int j0n = s.ci_next * CH;
    const int cnn = (M - j0n) < CH ? (M - j0n) : CH;
    float *img = c.sm + (size_t)(1 - cur) * c.buf_floats;
    knn_f16_store_chunk<T::DK>(img, CH, cnn, sc, c.mu, c.ptid, p.preg, p.stage_ev < nchunk ? c.nall + (size_t)p.stage_ev * CH : nullptr,
                               p.stage_ev < nchunk && c.nallm ? c.nallm + (size_t)p.stage_ev * CH : nullptr,
                               reinterpret_cast<const float *>(c.cmax + 1), p.pmax, p.pnan);
    if (p.stage_ev == nchunk - 1) knn_publish_pmax(c, p);  // last phase-A chunk
    ++p.stage_ev;
    if (p.stage_ev < nevents) {
        const int cnx = p.stage_ev < nchunk ? p.stage_ev : 2 * nchunk - 2 - p.stage_ev;
        knn_f16_load_chunk<T::DK>(c.yb, c.a.D, cnx * CH, (M - cnx * CH) < CH ? (M - cnx * CH) : CH, CH, c.ptid, p.preg);
    }
}
// Float32 GEMM, producers: direct-to-LDS loads of the next chunk; norms in phase A, or whenever they are not kept
template <class T>
__device__ __forceinline__ void knn_mfma_stage_next_f32(const KnnMfmaCtx &c, const KnnStep &s, int cur) {
    const int M = c.a.M, CH = c.a.CH;
    const int j0n = s.ci_next * CH;
    const int cnn = (M - j0n) < CH ? (M - j0n) : CH;
    float *img = c.sm + (size_t)(1 - cur) * c.buf_floats;
    const bool phase_a = s.nstep1 < c.nchunk;
    knn_stage_chunk<T::DK>(c.yb, c.a.D, j0n, cnn, CH, img, c.a.keep_norms ? c.nall + (size_t)s.ci_next * CH : img + (size_t)CH * T::DP,
                           c.cmax, phase_a, phase_a || !c.a.keep_norms, c.vec4y, c.wv - kMWaves, c.lane);
}
// one step: the filter of this step's chunk and the staging of the next, by the waves the mode gives each
template <class T>
__device__ __forceinline__ void knn_mfma_chunk_step(const KnnMfmaCtx &c, const KnnStep &s, int cur, float sc, const KnnQueryOp<T> &qo,
                                                    KnnFilterOut &f, KnnProducer &p) {
    if (T::PRE) {  // all eight waves filter; the next chunk travels around it
        f32x4v creg[T::NCR];
        if (s.stage_next) knn_mfma_stage_request_pre<T>(c, s, cur, creg);
        if (c.wave_active) knn_mfma_filter<T>(c, s, cur, qo, f);
        if (s.stage_next) knn_mfma_stage_finish_pre<T>(c, cur, creg);
    } else if (c.consumer) {
        if (c.wave_active) knn_mfma_filter<T>(c, s, cur, qo, f);
    } else if (s.stage_next) {
        if (T::F16) knn_mfma_stage_next_f16<T>(c, s, cur, sc, p);
        else knn_mfma_stage_next_f32<T>(c, s, cur);
    }
}

// ---- tau and threshold (behind phase A)
__device__ __forceinline__ void knn_bitonic_merge32(float (&v)[32]) {  // a bitonic sequence of 32 -> ascending
#pragma unroll
    for (int j = 16; j > 0; j >>= 1) {
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const int l = i ^ j;
            if (l > i) {
                const float lo = vmin_f32(v[i], v[l]), hi = vmax_f32(v[i], v[l]);
                v[i] = lo;
                v[l] = hi;
            }
        }
    }
}
// tau: kk-th smallest of the group minima of every query (32 in this lane, 32 in its partner; PRE: as many again in the pair's
// other wave).  PRE: contains block barriers (every wave calls it); the exchange space becomes the lane lists behind them.
template <class T>
__device__ __forceinline__ float knn_mfma_tau(const KnnMfmaCtx &c, float (&mn)[32]) {
    const int h = c.h, jl = c.jl, wv = c.wv, kk = c.kk;
    if (T::PRE && kk <= 24 && c.a.M >= 128) {
        // 128 group minima per query in the layout of the D = 3 kernel (32 per lane x two half-lanes x the pair's two waves):
        // its reduced selection
        const float tau = knn_tau_8of16<kMWaves>(mn, reinterpret_cast<float *>(c.lists), wv, jl, h, kk);
        __syncthreads();
        return tau;
    }
    k3_sort_regs<32>(mn);
    float oth[32];
#pragma unroll
    for (int r = 0; r < 32; ++r) oth[r] = __shfl_xor(mn[31 - r], 32, 64);
#pragma unroll
    for (int r = 0; r < 32; ++r)  // half 0 keeps the 32 smallest of the 64 (a bitonic sequence)
        mn[r] = h ? vmax_f32(mn[r], oth[r]) : vmin_f32(mn[r], oth[r]);
    knn_bitonic_merge32(mn);
    if (T::PRE) {
        // the other wave of the pair holds the minima of the other tiles: the 32 smallest of the 128 through LDS (the
        // lane lists are not in use yet), one more bitonic merge
        float *xch = reinterpret_cast<float *>(c.lists);  // [2 kMWaves][32][33]
        if (h == 0) {
#pragma unroll
            for (int r = 0; r < 32; ++r) xch[(wv * 32 + jl) * 33 + r] = mn[r];
        }
        __syncthreads();
        const float *po = xch + (((wv + kMWaves) % (2 * kMWaves)) * 32 + jl) * 33;
#pragma unroll
        for (int r = 0; r < 32; ++r) mn[r] = vmin_f32(mn[r], po[31 - r]);
        knn_bitonic_merge32(mn);
        __syncthreads();
    }
    float val = mn[0];
#pragma unroll
    for (int r = 1; r < 32; ++r) val = (kk - 1) == r ? mn[r] : val;
    return __shfl(val, jl, 64);  // kk <= 32: always among the 32 smallest (half 0)
}
// thr = tau + twice the filter's error bound for this query (NaN / inf => the exact merge)
template <class T>
__device__ __forceinline__ float knn_mfma_threshold(const KnnMfmaCtx &c, const KnnQueryOp<T> &qo, float funit, float tau) {
    const int D = c.a.D;
    const float qn = qo.qn;
    const float c2 = __builtin_bit_cast(float, *c.cmax);
    float eps;
    if (T::F16) {
        // scaled units (c~ = sc c, |c~| < 1; qn = |sc q|^2): the rounded operands differ by 2^-11 relative each,
        // sum |c~_d a_d| <= 2 |c~||q~| <= qn + c2; fp32 accumulation, the oracle's own (D+2) u, fp16 underflow floor
        // |F^ - (sc^2 d_oracle - qn)| <= A (n_c + qn) + floor for candidate c with scaled norm n_c (A = acoef_q).
        // two_norms: the candidate's share A n_c is already inside the norms (upwards in phase A, downwards
        // in phase B), the query keeps B_q = A qn + floor_q: a far candidate no longer widens everybody's
        // band.  Otherwise n_c <= c2 for all of them.
        const float acoef_q = 8.0f * (float)(4 * D + 8) * 0x1p-24f + 0x1.01p-10f;
        const float floor_q = 0x1p-24f * sqrtf((float)D) * (qn / funit + 2.0f * funit);
        eps = c.a.two_norms ? acoef_q * qn + floor_q : acoef_q * (qn + c2) + floor_q + 0x1p-26f * sqrtf((float)D) * c2 / funit;
        eps = (qo.qok && c2 == c2) ? eps : INFINITY;  // c2 is NaN for a non-finite / overflow-prone cloud (scale pass)
    } else {
        eps = (8.0f * (float)(D + 4) * 0x1p-24f) * (qn + c2);
        eps = qn + c2 < 1.0e38f ? eps : INFINITY;  // (|q| + |c|)^2 <= 2 (qn + c2): no exact distance overflows
    }
    float thr = tau + 2.0f * eps;
    // Phase B of the fp16 filters starts the accumulators at n_c - thr and keeps the SIGN of the result (one v_alignbit per row
    // where a compare costs v_cmp + v_cndmask + v_or and two wait states).  The accumulation then carries thr through its D + 1
    // roundings: against the compare form the result moves by at most (D + 1) u (2 n_c + |thr| + 2 sum |products|)
    // (65 u (4 n_c + 2 qn + |thr|) at D = 64), u = 2^-24.  The candidate's and the query's own shares sit inside the budget the
    // filter already grants them (8 (4 D + 8) u = 2112 u each at D = 64, of which the compare form uses ~130 u); the threshold's
    // share, (K + 1) u |thr| with K = D products (K = 3 D on the Float32 GEMM, whose compare form does not need it), is added
    // here four times over -- at D = 64 2^-16 |thr|, 1/64 of the band of a candidate at the boundary (its norm is of the
    // threshold's size) -- and it makes the test strict (a candidate at the threshold gives a negative result, never +-0).
    thr = thr + (4.0f * (float)((T::F16 ? 1 : 3) * D + 1) * 0x1p-24f) * (fabsf(thr) + qn);
    return thr;
}

// ---- exact phase.  What the phases share per lane:
struct KnnSurvivors {
    int n;                       // survivors of the lane's query
    bool fast;                   // they fit the key arrays: ranked by the block's fast path
    bool handled;                // answered by the medium path
    unsigned long long dpk[4];   // PRE: the four parts' packed per-stage counts
    int mystart, mycount;        // this lane's share of the ids (the query's four lanes split them)
};
// (1) list counts and path flags.  Contains the barrier behind which the chunk buffers are free: they hold the keys.
template <class T>
__device__ __forceinline__ void knn_mfma_list_counts(const KnnMfmaCtx &c, const KnnFilterOut &f, KnnSurvivors &sv) {
    constexpr int LCAP = T::LCAP;
    const int cw = c.cw, jl = c.jl, h = c.h, lane = c.lane, srl = c.a.srl, cnt = f.cnt;
    const int need = c.kk < c.a.M ? c.kk : c.a.M;
    if (T::PRE) {
        // every lane publishes the per-stage counts of its own list (bytes of a 64-bit word; srl == 0: the total in byte 0)
        // and whether the list overflowed (top bit: a stage holds < 128 survivors of the <= 64 that matter)
        const int nv = cnt < LCAP - 1 ? cnt : LCAP - 1;
        const int tsh = srl > 0 ? srl - 5 : 31;
        unsigned long long pk = 0;
        int totx = 0;
        if (srl > 0) {
            for (int e = 0; e < nv; ++e) {
                const unsigned int w = (unsigned int)f.mylist[e * 64];
                const int pc = __builtin_popcount(w & 0xffffu);
                totx += pc;
                pk += (unsigned long long)pc << (((w >> 16) >> tsh) * 8);
            }
        } else {  // no row stages (column slices, gather): the total phase B counted -- no walk over the list (a chain of LDS round trips)
            totx = f.totb;
            pk = (unsigned long long)(unsigned int)f.totb;
        }
        // (the bytes are only meaningful while none can carry: a part with more than 63 survivors -- the query is not a fast one
        //  then -- publishes its plain total behind a marker bit instead)
        c.qpk[(cw * 32 + jl) * 4 + c.part] = (totx <= 63 ? pk : (1ull << 62) | (unsigned long long)totx) | (cnt > LCAP - 1 ? 1ull << 63 : 0ull);
        c.lcnt2[c.wv * 64 + lane] = (unsigned short)nv;
    } else if (c.consumer) {
        const int nv = cnt < kMLCap - 1 ? cnt : kMLCap - 1;
        int tot = 0;
        for (int e = 0; e < nv; ++e) tot += __builtin_popcount((unsigned int)f.mylist[e * 64] & 0xffffu);
        const int totp = __shfl_xor(tot, 32, 64);
        const int cntp = __shfl_xor(cnt, 32, 64);
        const int n = tot + totp;
        const bool lists_ok = c.wave_active && c.qi < c.a.N && f.thr < INFINITY && cnt <= kMLCap - 1 && cntp <= kMLCap - 1 && n >= need;
        const bool fast = lists_ok && n <= kMKeyCap;
        const bool medium = lists_ok && n > kMKeyCap && n <= kMMedCap;  // too many for the key arrays, lists intact
        c.lcnt[cw * 64 + lane] = (h ? totp : 0) | (nv << 16);  // start offset of this lane's ids | entries
        if (h == 0) { c.qn_n[cw * 32 + jl] = n; c.qflag[cw * 32 + jl] = fast ? 1 : (medium ? 2 : 0); c.qbelow[cw * 32 + jl] = 0; }
    }
    __syncthreads();
    KNN_PROBE_MARK(21);
    sv.n = c.qn_n[cw * 32 + jl];
    sv.fast = c.qflag[cw * 32 + jl] == 1;
    sv.handled = c.qflag[cw * 32 + jl] == 2;
#pragma unroll
    for (int q = 0; q < 4; ++q) sv.dpk[q] = 0ull;
    if (T::PRE) {
        bool ovf = false, big = false;
        int tot4 = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned long long v = c.qpk[(cw * 32 + jl) * 4 + q];
            ovf |= (v >> 63) != 0;
            const bool bigp = ((v >> 62) & 1ull) != 0;  // more than 63 survivors in this part alone: its plain total
            big |= bigp;
            sv.dpk[q] = bigp ? 0ull : v & ~(3ull << 62);
            tot4 += bigp ? (int)(unsigned int)v : (int)((sv.dpk[q] * 0x0101010101010101ull) >> 56);  // sum of the bytes
        }
        sv.n = tot4;
        const bool lists_ok = c.wave_active && c.qi < c.a.N && f.thr < INFINITY && !ovf && sv.n >= need;
        sv.fast = lists_ok && !big && sv.n <= kMKeyCap;
        sv.handled = lists_ok && !sv.fast && sv.n <= kMMedCap;
        if (c.part == 0) { c.qn_n[cw * 32 + jl] = sv.n; c.qflag[cw * 32 + jl] = sv.fast ? 1 : (sv.handled ? 2 : 0); c.qbelow[cw * 32 + jl] = 0; }
    }
}
// the key arrays of the lane's query, in the chunk buffers: distance bits, indices (stride kMKeyStride, sentinels behind the n keys)
__device__ __forceinline__ unsigned int *knn_mfma_qd(const KnnMfmaCtx &c, int q) { return reinterpret_cast<unsigned int *>(c.sm) + (size_t)q * kMKeyStride; }
__device__ __forceinline__ int *knn_mfma_qj(const KnnMfmaCtx &c, int q) {
    return reinterpret_cast<int *>(c.sm) + (size_t)kMWaves * 32 * kMKeyStride + (size_t)q * kMKeyStride;
}
// rank slots of a query, in the (dead) lane lists: [32 + 1 pad] keys
__device__ __forceinline__ unsigned long long *knn_mfma_slots(const KnnMfmaCtx &c, int q) {
    return reinterpret_cast<unsigned long long *>(c.lists) + (size_t)q * 33;
}

// exact phase, before the lists are decoded: the thread's first share of the candidate rows is requested (the first row stage,
// or the first column slice), so that it arrives meanwhile; returns the thread's place in a row stage.  (D > 64: the rows are
// staged and evaluated in two column halves of <= 64 dimensions; column slices exist for D <= 64 only, knn_mfma_plan.)
struct KnnStageGeo {
    int DS;          // staged width of a row (half), floats
    int RPI;         // rows per sweep of the block (DS / 4 divides the block size)
    int srow, scol;  // the thread's first row and its column
};
template <class T>
__device__ __forceinline__ KnnStageGeo knn_mfma_exact_prefetch(const KnnMfmaCtx &c, f32x4v (&sreg)[8]) {
    const int D = c.a.D, M = c.a.M, srl = c.a.srl, tid = c.tid;
    KnnStageGeo g;
    g.DS = T::DP > 64 && D > 64 ? 64 : D;
    const int PR = g.DS >> 2;
    g.RPI = srl > 0 ? kMThreads / PR : 0;
    g.srow = srl > 0 ? tid / PR : 0;
    g.scol = (tid - g.srow * PR) * 4;
    if (srl > 0) knn_stage_fetch(c.yb, D, M, 0, g.srow, g.RPI, g.scol, sreg);
    // column slices: rows (tid >> 2) + 128 i, piece tid & 3
    if constexpr (T::DP <= 64)
        if (c.a.csl > 0) knn_stage_fetch(c.yb, D, M, 0, tid >> 2, kMThreads / 4, 4 * (tid & 3), sreg);
    return g;
}

// ---- medium path (tight clusters, many duplicates: more candidates inside the band than the key arrays hold):
//      the wave decodes the query's lane lists into an id list and selects exactly among those ids,
//      instead of scanning all M candidates in the fallback.  The lists are intact until the barrier after the decode.
template <class T>
__device__ __forceinline__ void knn_mfma_medium_path(const KnnMfmaCtx &c, const KnnSurvivors &sv) {
    constexpr bool PRE = T::PRE;
    constexpr int LCAP = T::LCAP;
    const int cw = c.cw, lane = c.lane, D = c.a.D, k = c.a.k, drop = c.a.drop;
    if (!c.wave_active) return;
    const unsigned long long mmask = __ballot(sv.handled);
    int *ids = c.med + c.wv * (kMMedCap + 128);
    for (unsigned int bm = (unsigned int)mmask | (unsigned int)(mmask >> 32); bm; bm &= bm - 1) {
        const int j = __builtin_ctz(bm);
        if ((j & 1) != (c.consumer ? 0 : 1)) continue;  // the pair's two waves share the queries
        int total = 0;
        for (int h2 = 0; h2 < (PRE ? 4 : 2); ++h2) {  // (PRE: h2 = 2 * (wave of the pair) + half-wave)
            const int src = (h2 & 1) * 32 + j;
            const int lw = PRE ? cw + kMWaves * (h2 >> 1) : cw;  // the wave that holds the list
            const int nv2 = PRE ? c.lcnt2[lw * 64 + src] : c.lcnt[cw * 64 + src] >> 16;
            const unsigned int w = lane < nv2 ? (unsigned int)c.lists[((PRE ? lw * LCAP : cw * kMLCap) + lane) * 64 + src] : 0u;  // nv2 < 64
            const int pc = __builtin_popcount(w & 0xffffu);
            int incl = pc;
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) {
                const int t = __shfl_up(incl, m, 64);
                if (lane >= m) incl += t;
            }
            int pos = total + incl - pc;
            unsigned int m16 = w & 0xffffu;
            const int rowbase = (int)(w >> 16) * 32 + 4 * (h2 & 1);
            while (m16) {
                const int r = __builtin_ctz(m16);
                m16 &= m16 - 1;
                ids[pos++] = rowbase + (r & 3) + 8 * (r >> 2);
            }
            total += __shfl(incl, 63, 64);
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
        float bd;
        int bj;
        knn_exact_bruteforce(c.xb + (size_t)(c.q0 + j) * D, c.yb, total, D, c.kk, lane, reinterpret_cast<float *>(ids + kMMedCap),
                             ids + kMMedCap + 64, bd, bj, ids);
        const int r = lane - drop;
        if (r >= 0 && r < k) {
            c.a.idx[((size_t)c.b * c.a.N + c.q0 + j) * k + r] = bj;
            if (c.a.dist) c.a.dist[((size_t)c.b * c.a.N + c.q0 + j) * k + r] = bd;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// ---- (2) decode: the lanes of a fast query turn their mask words into candidate ids (integer work only).  srl > 0 (staged
//      exact phase): the ids of a query are grouped by row stage (2^srl candidate rows, at most 8 stages): per-stage counts of
//      the lane lists in the bytes of a 64-bit word (n <= 60 < 256), prefix sums by one multiplication.
// one lane's list: nv words, four in flight; startpk byte s: where this lane's ids of stage s go (staged), else byte 0: the next id
template <int LCAP>
__device__ __forceinline__ void knn_decode_list(const int *mylist, int nv, int h, bool staged, int tsh, unsigned long long startpk, int *qj) {
    for (int e0 = 0; e0 < nv; e0 += 4) {
        unsigned int w[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) w[u] = (unsigned int)mylist[(e0 + u < LCAP ? e0 + u : LCAP - 1) * 64];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            unsigned int m = e0 + u < nv ? (w[u] & 0xffffu) : 0u;
            const int rowbase = (int)(w[u] >> 16) * 32 + 4 * h;
            const int sh = staged ? (int)((w[u] >> 16) >> tsh) * 8 : 0;
            int pos = (int)(startpk >> sh) & 0xff;
            startpk += (unsigned long long)__builtin_popcount(m) << sh;
            while (m) {
                const int r = __builtin_ctz(m);
                m &= m - 1;
                qj[pos++] = rowbase + (r & 3) + 8 * (r >> 2);
            }
        }
    }
}
__device__ __forceinline__ void knn_key_sentinels(unsigned int *qd, int *qj, int n) {  // for the b128 sweeps
    qd[n] = 0xffffffffu; qd[n + 1] = 0xffffffffu; qd[n + 2] = 0xffffffffu;
    qj[n] = 0x7fffffff; qj[n + 1] = 0x7fffffff; qj[n + 2] = 0x7fffffff;
}
template <class T>
__device__ __forceinline__ void knn_mfma_decode(const KnnMfmaCtx &c, const KnnFilterOut &f, const KnnSurvivors &sv, unsigned int *qd, int *qj) {
    constexpr int LCAP = T::LCAP;
    const int srl = c.a.srl, h = c.h, cw = c.cw, jl = c.jl, lane = c.lane, n = sv.n;
    if (T::PRE) {
        if (sv.fast) {  // every one of the query's four lanes decodes its own list behind the lists of the parts before it
            const int nv = c.lcnt2[c.wv * 64 + lane];
            const unsigned long long incl = (sv.dpk[0] + sv.dpk[1] + sv.dpk[2] + sv.dpk[3]) * 0x0101010101010101ull;  // byte s: survivors in stages 0..s
            unsigned long long before = 0;
#pragma unroll
            for (int q = 0; q < 3; ++q) before += q < c.part ? sv.dpk[q] : 0ull;
            unsigned long long startpk = (srl > 0 ? incl << 8 : 0ull) + before;  // byte s: where this lane's ids of stage s go
            const int tsh = srl > 0 ? srl - 5 : 31;
            knn_decode_list<LCAP>(f.mylist, nv, h, srl > 0, tsh, startpk, qj);
            if (c.part == 3) knn_key_sentinels(qd, qj, n);
        }
    } else if (c.consumer && sv.fast) {
        const int meta = c.lcnt[cw * 64 + lane];
        const int nv = meta >> 16;
        if (srl > 0) {
            const int tsh = srl - 5;  // tile -> stage
            unsigned long long pk = 0;
            for (int e = 0; e < nv; ++e) {
                const unsigned int w = (unsigned int)f.mylist[e * 64];
                pk += (unsigned long long)__builtin_popcount(w & 0xffffu) << (((w >> 16) >> tsh) * 8);
            }
            const unsigned long long pko = ((unsigned long long)(unsigned int)__shfl_xor((int)(pk >> 32), 32, 64) << 32) |
                                           (unsigned int)__shfl_xor((int)pk, 32, 64);
            const unsigned long long incl = (pk + pko) * 0x0101010101010101ull;  // byte s: survivors in stages 0..s
            if (h == 0) c.qstpk[cw * 32 + jl] = incl;
            knn_decode_list<kMLCap>(f.mylist, nv, h, true, tsh, (incl << 8) + (h ? pko : 0ull), qj);
        } else {
            knn_decode_list<kMLCap>(f.mylist, nv, h, false, 0, (unsigned long long)(meta & 0xffff), qj);
        }
        if (h) knn_key_sentinels(qd, qj, n);
    }
}

// ---- (3) exact distances of a fast query's ids: the oracle's, same operations in the same order in all three forms below.
// The query's survivors are split over its four lanes (two halves x consumer / producer wave).
// Column slices: ALL candidate rows pass through LDS, 16 dimensions at a time (csl = D / 16 slices), as four planes of 16-byte
// pieces ([piece c][row], plane stride 16 Mp + 32 bytes: the coalesced staging writes and the reads of consecutive rows are
// conflict-free).  In every slice the four lanes of a query share ALL its survivors evenly -- the row stages below share the
// survivors of one stage at a time: ~1.7 per lane against a fullest lane of 3-4 (42 % of the lane slots held a pair); whole
// queries differ far less (27 +- 5 survivors) -- and a pair's running sum waits in a register between slices: the oracle's order
// of additions.  The query's slice is 16 floats in registers, the next slice's pieces of rows and query are in flight while this
// one is summed.
__device__ __forceinline__ void knn_mfma_exact_slices(const KnnMfmaCtx &c, const KnnSurvivors &sv, f32x4v (&sreg)[8], unsigned int *qd,
                                                      const int *qj) {
    const int M = c.a.M, D = c.a.D, csl = c.a.csl, tid = c.tid;
    const int MPc = (M + kMThreads / 4 - 1) / (kMThreads / 4) * (kMThreads / 4);
    const int PS = MPc * 4 + 8;  // plane stride, floats
    float *stg = reinterpret_cast<float *>(c.lists);
    const bool act = c.wave_active && sv.fast;
    const int crow = tid >> 2, cc = tid & 3;
    const float *qrow = c.xb + (size_t)(act ? c.qi : 0) * D;
    f32x4v qs[4], qnx[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) qs[t] = *reinterpret_cast<const f32x4v *>(qrow + 4 * t);
    // this lane's pairs stay in registers across the slices: the candidate's plane offset and the running sum (n <= 64 survivors per
    // query: at most 16 per lane); four pairs are in flight -- their 16 pieces are requested together, their four chains of additions
    // interleave (a slice of ONE pair is 16 dependent additions: two pairs in flight left the phase latency bound, 2.5 us per slice)
    const int cnt_l = act ? sv.mycount : 0;
    int jo[16];
    float acc[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        jo[u] = u < cnt_l ? qj[sv.mystart + u] * 4 : 0;
        acc[u] = 0.0f;
    }
    for (int s = 0; s < csl; ++s) {
        if (s) __syncthreads();  // every lane is done with the previous slice
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int row = crow + i * (kMThreads / 4);
            if (row < MPc) *reinterpret_cast<f32x4v *>(stg + (size_t)cc * PS + (size_t)row * 4) = sreg[i];
        }
        __syncthreads();
        if (s < 3) KNN_PROBE_MARK(26 + 2 * s);
        if (s + 1 < csl) {
            knn_stage_fetch(c.yb, D, M, 0, crow, kMThreads / 4, 16 * (s + 1) + 4 * cc, sreg);
#pragma unroll
            for (int t = 0; t < 4; ++t) qnx[t] = *reinterpret_cast<const f32x4v *>(qrow + 16 * (s + 1) + 4 * t);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            if (__ballot(4 * g < cnt_l) != 0ull) {  // (wave-uniform: some lane still has a pair in this group)
                f32x4v cv[4][4];
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int t = 0; t < 4; ++t) cv[e][t] = *reinterpret_cast<const f32x4v *>(stg + jo[4 * g + e] + t * PS);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    f32x4v m[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const f32x4v d = qs[t] - cv[e][t];
                        m[e] = d * d;
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[4 * g + e] = acc[4 * g + e] + m[e].x;
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[4 * g + e] = acc[4 * g + e] + m[e].y;
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[4 * g + e] = acc[4 * g + e] + m[e].z;
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[4 * g + e] = acc[4 * g + e] + m[e].w;
                }
            }
        }
        if (s < 3) KNN_PROBE_MARK(27 + 2 * s);
#pragma unroll
        for (int t = 0; t < 4; ++t) qs[t] = qnx[t];
    }
#pragma unroll
    for (int u = 0; u < 16; ++u)
        if (u < cnt_l) qd[sv.mystart + u] = __builtin_bit_cast(unsigned int, acc[u]);
}
// Row stages: the candidate rows come through LDS one stage (2^srl rows) at a time, loaded coalesced once per block (every row
// exactly once: M * 4D bytes from L2 instead of 4D per survivor), rows 16 bytes apart in the banks.  Per stage the four lanes of
// a query split its survivors of that stage; the query row sits in registers.
// One pass over the stages for the columns [hoff, hoff + wdt) -- store the stage, fetch the next, split the stage's survivors,
// pair loop.  HALVES (D > 64): a 128-dimension query row is 128 registers -- with the stage registers and the pair buffers the
// kernel spilled 330-380 of them.  The pass runs once per column half instead: dimensions 0..63 of every row are staged and
// summed first (the partial sum waits in the pair's distance slot), then (hf = 1) 64..D-1 continue it -- the oracle's order;
// each half is the D = 64 pass (same stage size, same traffic).
template <int QW, bool HALVES>
__device__ __forceinline__ void knn_mfma_row_stage_pass(const KnnMfmaCtx &c, const KnnStageGeo &g, const KnnSurvivors &sv, unsigned long long incl,
                                                        bool act, int hf, int nhalf, int hoff, int wdt, f32x4v (&sreg)[8], unsigned int *qd,
                                                        const int *qj) {
    const int D = c.a.D, M = c.a.M, srl = c.a.srl;
    const int SRW = 1 << srl, RSX = g.DS + 4;
    float *stg = reinterpret_cast<float *>(c.lists);
    const int nstage = (M + SRW - 1) >> srl;
    const int srow = g.srow, scol = g.scol, RPI = g.RPI, part = c.part;
    f32x4v qreg[QW / 4];
    {
        const float *qrow = c.xb + (size_t)(act ? c.qi : 0) * D + hoff;
#pragma unroll
        for (int t = 0; t < QW / 4; ++t)
            qreg[t] = 4 * t < wdt ? *reinterpret_cast<const f32x4v *>(qrow + 4 * t) : f32x4v{0.f, 0.f, 0.f, 0.f};
    }
    for (int s = 0; s < nstage; ++s) {
        if (s || hf) __syncthreads();  // every lane is done with the previous stage
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int row = srow + i * RPI;
            if (row < SRW) *reinterpret_cast<f32x4v *>(stg + (size_t)row * RSX + scol) = sreg[i];
        }
        __syncthreads();
        if (s < 3 && hf == 0) KNN_PROBE_MARK(26 + 2 * s);
        // the next stage of this half, or the first stage of the second half, in flight while this one is evaluated
        // (a half narrower than 64 columns: the pieces beyond it re-read its last piece and are never used)
        if (s + 1 < nstage) {
            knn_stage_fetch(c.yb + hoff, D, M, (s + 1) << srl, srow, RPI, HALVES ? (scol < wdt ? scol : wdt - 4) : scol, sreg);
        } else if (HALVES && hf + 1 < nhalf) {
            knn_stage_fetch(c.yb + 64, D, M, 0, srow, RPI, scol < D - 64 ? scol : D - 68, sreg);
        }
        if (act) {
            const int start = s ? (int)(incl >> (8 * (s - 1))) & 0xff : 0, end = (int)(incl >> (8 * s)) & 0xff;
            const int per = (end - start + 3) >> 2;
            const int a0 = start + part * per < end ? start + part * per : end;
            const int a1 = a0 + per < end ? a0 + per : end;
            for (int p0 = a0; p0 < a1; p0 += 2) {
                const bool two = p0 + 1 < a1;
                const float *cp0 = stg + (size_t)(qj[p0] - (s << srl)) * RSX;
                const float *cp1 = stg + (size_t)(qj[two ? p0 + 1 : p0] - (s << srl)) * RSX;
                float s0 = hf ? __builtin_bit_cast(float, qd[p0]) : 0.0f;
                float s1 = hf && two ? __builtin_bit_cast(float, qd[p0 + 1]) : 0.0f;
                if (wdt == QW) knn_pair_dist<QW, true>(qreg, cp0, cp1, wdt, s0, s1);
                else knn_pair_dist<QW, false>(qreg, cp0, cp1, wdt, s0, s1);
                qd[p0] = __builtin_bit_cast(unsigned int, s0);
                if (two) qd[p0 + 1] = __builtin_bit_cast(unsigned int, s1);
            }
        }
        if (s < 3 && hf == 0) KNN_PROBE_MARK(27 + 2 * s);
    }
}
template <class T>
__device__ __forceinline__ void knn_mfma_exact_row_stages(const KnnMfmaCtx &c, const KnnStageGeo &g, const KnnSurvivors &sv, f32x4v (&sreg)[8],
                                                          unsigned int *qd, const int *qj) {
    constexpr int DP = T::DP;
    const int D = c.a.D;
    const bool act = c.wave_active && sv.fast;
    const unsigned long long incl = !act ? 0ull : (T::PRE ? (sv.dpk[0] + sv.dpk[1] + sv.dpk[2] + sv.dpk[3]) * 0x0101010101010101ull
                                                         : c.qstpk[c.cw * 32 + c.jl]);
    if constexpr (DP <= 64) {
        knn_mfma_row_stage_pass<DP, false>(c, g, sv, incl, act, 0, 1, 0, D, sreg, qd, qj);
    } else {
        const int nhalf = D > 64 ? 2 : 1;
        for (int hf = 0; hf < nhalf; ++hf)  // this half's first column and width
            knn_mfma_row_stage_pass<64, true>(c, g, sv, incl, act, hf, nhalf, 64 * hf, hf ? D - 64 : g.DS, sreg, qd, qj);
    }
}
// Gather (no staging: unaligned clouds, D % 4 != 0, or no room): the query row sits in registers; candidate rows are gathered
// from L2 one full 128-byte line per request (32 dimensions), two candidates in flight
template <class T>
__device__ __forceinline__ void knn_mfma_exact_gather(const KnnMfmaCtx &c, const KnnSurvivors &sv, unsigned int *qd, const int *qj) {
    constexpr int DP = T::DP;
    const int D = c.a.D, mystart = sv.mystart, mycount = sv.mycount;
    const float *yb = c.yb;
    const float *qrow = c.xb + (size_t)c.qi * D;
    if (c.vec4y && c.vec4x) {
        constexpr int QR = DP > 64 ? 1 : DP / 4;  // D > 64: the query pieces are re-read (L1) with every 32-dimension block
        float4 qreg[QR];
        if (DP <= 64) {
#pragma unroll
            for (int t = 0; t < QR; ++t)
                qreg[t] = 4 * t < D ? *reinterpret_cast<const float4 *>(qrow + 4 * t) : float4{0.f, 0.f, 0.f, 0.f};
        }
        for (int p0 = mystart; p0 < mystart + mycount; p0 += 2) {
            const bool two = p0 + 1 < mystart + mycount;
            const float *cp0 = yb + (size_t)qj[p0] * D;
            const float *cp1 = yb + (size_t)qj[two ? p0 + 1 : p0] * D;
            float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
            for (int d0 = 0; d0 < DP; d0 += 32) {
                if (d0 < D) {
                    float4 c0[8], c1[8], q8[DP > 64 ? 8 : 1];
#pragma unroll
                    for (int t = 0; t < 8; ++t)
                        if (d0 + 4 * t < D) {
                            c0[t] = *reinterpret_cast<const float4 *>(cp0 + d0 + 4 * t);
                            c1[t] = *reinterpret_cast<const float4 *>(cp1 + d0 + 4 * t);
                            if (DP > 64) q8[t] = *reinterpret_cast<const float4 *>(qrow + d0 + 4 * t);
                        }
#pragma unroll
                    for (int t = 0; t < 8; ++t)
                        if (d0 + 4 * t < D) {
                            const float4 qv = DP > 64 ? q8[DP > 64 ? t : 0] : qreg[DP > 64 ? 0 : d0 / 4 + t];
                            float t0 = qv.x - c0[t].x, t1 = qv.y - c0[t].y, t2 = qv.z - c0[t].z, t3 = qv.w - c0[t].w;
                            s0 = s0 + t0 * t0;
                            s0 = s0 + t1 * t1;
                            s0 = s0 + t2 * t2;
                            s0 = s0 + t3 * t3;
                            t0 = qv.x - c1[t].x; t1 = qv.y - c1[t].y; t2 = qv.z - c1[t].z; t3 = qv.w - c1[t].w;
                            s1 = s1 + t0 * t0;
                            s1 = s1 + t1 * t1;
                            s1 = s1 + t2 * t2;
                            s1 = s1 + t3 * t3;
                        }
                }
            }
            qd[p0] = __builtin_bit_cast(unsigned int, s0);
            if (two) qd[p0 + 1] = __builtin_bit_cast(unsigned int, s1);
        }
    } else {
        for (int p0 = mystart; p0 < mystart + mycount; ++p0) {
            const float *cp = yb + (size_t)qj[p0] * D;
            float sd = 0.0f;
            for (int d = 0; d < D; ++d) {
                const float t = qrow[d] - cp[d];
                sd = sd + t * t;
            }
            qd[p0] = __builtin_bit_cast(unsigned int, sd);
        }
    }
}
// the form is chosen by shape (knn_mfma_plan: csl, srl)
template <class T>
__device__ __forceinline__ void knn_mfma_exact_distances(const KnnMfmaCtx &c, const KnnStageGeo &g, KnnSurvivors &sv, f32x4v (&sreg)[8],
                                                         unsigned int *qd, const int *qj) {
    const int per = (sv.n + 3) >> 2;
    sv.mystart = c.part * per < sv.n ? c.part * per : sv.n;
    sv.mycount = (sv.mystart + per <= sv.n ? per : sv.n - sv.mystart);
    bool slices = false;
    if constexpr (T::DP <= 64) slices = c.a.csl > 0;  // (the plan gives column slices to D <= 64 only: not compiled for DK = 4)
    if (slices) knn_mfma_exact_slices(c, sv, sreg, qd, qj);
    else if (c.a.srl > 0) knn_mfma_exact_row_stages<T>(c, g, sv, sreg, qd, qj);
    else if (c.wave_active && sv.fast) knn_mfma_exact_gather<T>(c, sv, qd, qj);
}

// ---- (4) rank on the distance bits (squared distances are >= +0: unsigned order), verified as in knn_f16_d3_kernel.  Passes of
//      eight of the lane's entries against all n keys; a remainder of at most four / two entries in every lane of the wave takes
//      a narrower pass (n = 33 ... 36 survivors -- nine entries per lane -- would cost a second full pass otherwise, 1152 instead
//      of 720 operations).
template <int W>
__device__ __forceinline__ void knn_rank_pass(const unsigned int *qd, const int *qj, unsigned long long *slots, int mystart, int myc, int nloop,
                                              int kk, int e0, int &below) {
    unsigned int md[W];
    int rank[W];
#pragma unroll
    for (int u = 0; u < W; ++u) {
        md[u] = e0 + u < myc ? qd[mystart + e0 + u] : 0xffffffffu;
        rank[u] = 0;
    }
    for (int i = 0; i < nloop; i += 4) {  // (nloop: n for the lanes of a fast query, 0 for the others)
        const uint4 o = *reinterpret_cast<const uint4 *>(qd + i);
#pragma unroll
        for (int u = 0; u < W; ++u) {  // compare + add-with-carry: two VALU ops per pair
            unsigned long long cc;
            asm("v_cmp_lt_u32_e64 %1, %2, %3\n\tv_addc_co_u32_e64 %0, %1, 0, %0, %1" : "+v"(rank[u]), "=&s"(cc) : "v"(o.x), "v"(md[u]));
            asm("v_cmp_lt_u32_e64 %1, %2, %3\n\tv_addc_co_u32_e64 %0, %1, 0, %0, %1" : "+v"(rank[u]), "=&s"(cc) : "v"(o.y), "v"(md[u]));
            asm("v_cmp_lt_u32_e64 %1, %2, %3\n\tv_addc_co_u32_e64 %0, %1, 0, %0, %1" : "+v"(rank[u]), "=&s"(cc) : "v"(o.z), "v"(md[u]));
            asm("v_cmp_lt_u32_e64 %1, %2, %3\n\tv_addc_co_u32_e64 %0, %1, 0, %0, %1" : "+v"(rank[u]), "=&s"(cc) : "v"(o.w), "v"(md[u]));
        }
    }
#pragma unroll
    for (int u = 0; u < W; ++u)
        if (e0 + u < myc && rank[u] < kk) {
            slots[rank[u]] = ((unsigned long long)md[u] << 32) | (unsigned int)qj[mystart + e0 + u];
            below += 1 + (rank[u] << 8);
        }
}
__device__ __forceinline__ void knn_mfma_rank(const KnnMfmaCtx &c, const KnnSurvivors &sv, const unsigned int *qd, const int *qj,
                                              unsigned long long *slots) {
    const int myc = (c.wave_active && sv.fast) ? sv.mycount : 0;
    const int nloop = (c.wave_active && sv.fast) ? sv.n : 0;
    int below = 0;
    for (int e0 = 0;;) {
        const int rem = myc - e0;
        if (__ballot(rem > 0) == 0ull) break;
        if (__ballot(rem > 2) == 0ull) { knn_rank_pass<2>(qd, qj, slots, sv.mystart, myc, nloop, c.kk, e0, below); e0 += 2; }
        else if (__ballot(rem > 4) == 0ull) { knn_rank_pass<4>(qd, qj, slots, sv.mystart, myc, nloop, c.kk, e0, below); e0 += 4; }
        else { knn_rank_pass<8>(qd, qj, slots, sv.mystart, myc, nloop, c.kk, e0, below); e0 += 8; }
    }
    if (below) atomicAdd(&c.qbelow[c.cw * 32 + c.jl], below);
}

// ---- (5) output.  Verify (count and rank sum, see knn_f16_d3_kernel); slots [drop, kk) are the answer, in order: the query's
//      four lanes share the writes, 16 bytes at a time.  Returns whether the lane's query failed the check (an exact tie among its
//      first kk).
__device__ __forceinline__ bool knn_mfma_output(const KnnMfmaCtx &c, const KnnSurvivors &sv, const unsigned long long *slots) {
    const int k = c.a.k, drop = c.a.drop, kk = c.kk, part = c.part;
    int32_t *idx = c.a.idx;
    float *dist = c.a.dist;
    const bool bad = c.wave_active && c.qi < c.a.N && sv.fast && c.qbelow[c.cw * 32 + c.jl] != kk + ((kk * (kk - 1) / 2) << 8);  // (n >= kk here)
    if (c.wave_active && c.qi < c.a.N && sv.fast && !bad) {
        const size_t obase = ((size_t)c.b * c.a.N + c.qi) * k;
        if ((k & 3) == 0 && ((reinterpret_cast<uintptr_t>(idx) | (dist ? reinterpret_cast<uintptr_t>(dist) : 0)) & 15) == 0) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int v = part + 4 * u;
                if (4 * v < k) {
                    unsigned long long key[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) key[e] = slots[drop + 4 * v + e];
                    *reinterpret_cast<int4 *>(idx + obase + 4 * v) =
                        int4{(int)(unsigned int)key[0], (int)(unsigned int)key[1], (int)(unsigned int)key[2], (int)(unsigned int)key[3]};
                    if (dist)
                        *reinterpret_cast<float4 *>(dist + obase + 4 * v) =
                            float4{__builtin_bit_cast(float, (unsigned int)(key[0] >> 32)), __builtin_bit_cast(float, (unsigned int)(key[1] >> 32)),
                                   __builtin_bit_cast(float, (unsigned int)(key[2] >> 32)), __builtin_bit_cast(float, (unsigned int)(key[3] >> 32))};
                }
            }
        } else {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int r = drop + part + 4 * u;
                if (r < kk) {
                    const unsigned long long key = slots[r];
                    idx[obase + r - drop] = (int)(unsigned int)key;
                    if (dist) dist[obase + r - drop] = __builtin_bit_cast(float, (unsigned int)(key >> 32));
                }
            }
        }
    }
    return bad;
}

// ---- leftover merge, by the pair's two waves on alternate queries: tied queries are ranked again on the full keys, and the
//      leftovers (overflowing lists, non-finite bands) answered by the exact merge over all M candidates
__device__ __forceinline__ void knn_mfma_leftovers(const KnnMfmaCtx &c, const KnnSurvivors &sv, bool bad) {
    const int k = c.a.k, drop = c.a.drop, kk = c.kk, N = c.a.N, M = c.a.M, D = c.a.D, b = c.b, q0 = c.q0, lane = c.lane, cw = c.cw;
    int32_t *idx = c.a.idx;
    float *dist = c.a.dist;
    const bool slowq = c.qi < N && !sv.fast && !sv.handled;
    const unsigned long long badmask = __ballot(bad);
    const unsigned int bad32 = ((unsigned int)badmask | (unsigned int)(badmask >> 32)) & (c.consumer ? 0x55555555u : 0xaaaaaaaau);
    if (__builtin_popcount(bad32) <= 3) {
        // a few tied queries (ordinary data): the whole wave per query -- the quick form for a single one (knn_common.h)
        for (unsigned int bm = bad32; bm; bm &= bm - 1) {
            const int j = __builtin_ctz(bm);
            const int qs = cw * 32 + j;
            unsigned long long *sj = knn_mfma_slots(c, qs);
            knn_rank_ties(knn_mfma_qd(c, qs), knn_mfma_qj(c, qs), c.qn_n[qs], kk, sj, lane);
            for (int r = drop + lane; r < kk; r += 64) {
                const unsigned long long key = sj[r];
                idx[((size_t)b * N + q0 + j) * k + r - drop] = (int)(unsigned int)key;
                if (dist) dist[((size_t)b * N + q0 + j) * k + r - drop] = __builtin_bit_cast(float, (unsigned int)(key >> 32));
            }
        }
    } else {
        // many tied queries: the wave's tied queries at once, four lanes per query (knn_common.h: knn_rank_ties4)
        const int j = 2 * (lane >> 2) + (c.consumer ? 0 : 1), pl = lane & 3;
        const bool mine = ((bad32 >> j) & 1u) != 0;
        const int qs = cw * 32 + j;
        unsigned long long *sj = knn_mfma_slots(c, qs);
        knn_rank_ties4(knn_mfma_qd(c, qs), knn_mfma_qj(c, qs), mine ? c.qn_n[qs] : 0, kk, sj, pl);
        if (mine)
            for (int r = drop + pl; r < kk; r += 4) {
                const unsigned long long key = sj[r];
                idx[((size_t)b * N + q0 + j) * k + r - drop] = (int)(unsigned int)key;
                if (dist) dist[((size_t)b * N + q0 + j) * k + r - drop] = __builtin_bit_cast(float, (unsigned int)(key >> 32));
            }
    }
    // leftovers, wave-cooperative (scratch: behind all the slots)
    int *wscratch = reinterpret_cast<int *>(reinterpret_cast<unsigned char *>(c.lists) + kMSlotBytes) + c.wv * 128;
    const unsigned long long slowmask = __ballot(slowq);
    const unsigned int slow32 = (unsigned int)slowmask | (unsigned int)(slowmask >> 32);
    for (int j = c.consumer ? 0 : 1; j < 32; j += 2) {
        if (!((slow32 >> j) & 1u) || q0 + j >= N) continue;
        float bd;
        int bj;
        __builtin_amdgcn_wave_barrier();
        knn_exact_bruteforce(c.xb + (size_t)(q0 + j) * D, c.yb, M, D, kk, lane, reinterpret_cast<float *>(wscratch), wscratch + 64, bd, bj);
        const int r = lane - drop;
        if (r >= 0 && r < k) {
            idx[((size_t)b * N + q0 + j) * k + r] = bj;
            if (dist) dist[((size_t)b * N + q0 + j) * k + r] = bd;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// The kernel: the phases above in order.  Whatever the filter's predicates decide, every query's list equals the oracle's: the
// filter only chooses which candidates get an exact distance (a superset of the k + drop nearest), the rank check sends exact
// ties to the full-key ranking, and every query the fast path cannot answer goes to the exact merges.
template <int DK, KnnFilter MODE>
__global__ __launch_bounds__(kMThreads) void knn_mfma_kernel(KnnMfmaArgs a) {
    using T = KnnMfmaCfg<DK, MODE>;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    KnnMfmaCtx c;
    knn_mfma_coords<T>(a, sm, c);
    if (c.b >= a.B) return;
    KNN_PROBE_MARK(0);

    float sc, funit;
    knn_mfma_scale<T>(c, sc, funit);

    KnnQueryOp<T> qo;
    qo.qn = 0.0f;
    qo.qok = true;
    if (T::PRE) {
        float4 qv[T::NB16][2], mv[T::NB16][2];
        knn_mfma_query_load<T>(c, qv, mv);
        knn_mfma_first_chunk_request<T>(c);
        knn_mfma_query_operand_pre<T>(c, qv, mv, sc, qo);
    } else {
        knn_mfma_query_operand_lds<T>(c, sc, qo);
    }
    KNN_PROBE_MARK(1);

    KnnProducer prod;
    knn_mfma_first_chunk<T>(c, sc, prod);
    KNN_PROBE_MARK(2);

    KnnFilterOut f;
#pragma unroll
    for (int r = 0; r < 32; ++r) f.mn[r] = INFINITY;
    f.thr = 0.0f;
    f.cnt = 0;
    f.totb = 0;
    f.mylist = c.lists + (T::PRE ? c.wv * T::LCAP : c.cw * kMLCap) * 64 + c.lane;
    int cur = 0;  // buffer holding the chunk of this step
    for (int step = 0; step < 2 * c.nchunk; ++step) {
        const KnnStep s = knn_mfma_step(c, step);
        knn_mfma_chunk_step<T>(c, s, cur, sc, qo, f, prod);
        __syncthreads();
        KNN_PROBE_MARK(3 + step);
        if (s.stage_next) cur = 1 - cur;
        if (step == c.nchunk - 1 && (c.consumer || T::PRE)) f.thr = knn_mfma_threshold<T>(c, qo, funit, knn_mfma_tau<T>(c, f.mn));
    }
    KNN_PROBE_MARK(20);

    KnnSurvivors sv;
    knn_mfma_list_counts<T>(c, f, sv);
    f32x4v sreg[8];
    const KnnStageGeo geo = knn_mfma_exact_prefetch<T>(c, sreg);
    knn_mfma_medium_path<T>(c, sv);
    unsigned int *qd = knn_mfma_qd(c, c.cw * 32 + c.jl);
    int *qj = knn_mfma_qj(c, c.cw * 32 + c.jl);
    knn_mfma_decode<T>(c, f, sv, qd, qj);
    __syncthreads();  // ids visible to the producer partners; the lane lists are dead: their space holds the stages and the slots
    KNN_PROBE_MARK(22);
    knn_mfma_exact_distances<T>(c, geo, sv, sreg, qd, qj);
    __syncthreads();
    KNN_PROBE_MARK(23);
    unsigned long long *slots = knn_mfma_slots(c, c.cw * 32 + c.jl);
    knn_mfma_rank(c, sv, qd, qj, slots);
    __syncthreads();
    KNN_PROBE_MARK(24);
    const bool bad = knn_mfma_output(c, sv, slots);
    if (!c.wave_active) return;
    knn_mfma_leftovers(c, sv, bad);
    KNN_PROBE_MARK(25);
}

// ---- host: pre-pass predicates, LDS plan, launch ------------------------------------------------------------------------------
int knn_mfma_dp(int D) { return (D + 31) / 32 * 32 == 96 ? 128 : (D + 31) / 32 * 32; }  // padded feature dimension: DK = 1, 2, 4

constexpr size_t kMLdsMax = 152 * 1024;  // the kernels' opt-in limit of dynamic LDS

struct KnnMfmaPlan {
    int CH, img, keep_norms, two_norms, srl, csl;  // KnnMfmaArgs' fields of the same names
    size_t lds;
};
// f16: the fp16 filter; use_pre: behind the pre-pass; aligned16: x and y are 16-byte aligned
KnnMfmaPlan knn_mfma_plan(int DP, bool f16, bool use_pre, int M, int D, bool aligned16) {
    KnnMfmaPlan p{};
    const int RS = DP + 4, RSI = f16 ? DP / 2 : DP;
    const KnnMfmaLds L = KnnMfmaLds::make(DP);
    const size_t small = L.small();  // the fixed-size bookkeeping; the tail behind it is free for the exact phase's stages
    p.keep_norms = M <= 4096;  // all candidate norms stay in LDS: phase B does not recompute them
    // fp16 filter, room permitting: a second norms array (the candidate's error share folded in, upwards / downwards)
    p.two_norms = f16 && p.keep_norms && M <= 2048;
    const size_t fixed = L.bytes(M, p.keep_norms + p.two_norms);
    const size_t budget = 150 * 1024 - fixed;                                  // floats*4 for the two chunk buffers
    int CH = (int)(budget / 2 / ((size_t)RSI * 4 + 4)) / 64 * 64;
    if (CH > 256) CH = 256;
    if (f16 && !use_pre && CH > kMUnits * kMProd * 8 / DP / 64 * 64) CH = kMUnits * kMProd * 8 / DP / 64 * 64;  // producer register budget
    const int mpad = (M + 63) / 64 * 64;
    if (CH > mpad) CH = mpad;
    if (use_pre) CH = CH >= 256 ? 256 : (CH >= 128 ? 128 : 64);  // chunks tile the image's 256-row padding exactly
    p.CH = CH;
    size_t img = 2 * ((size_t)CH * RSI + CH);                                  // floats
    const size_t qstage = (size_t)kMWaves * 32 * RS;                           // prologue: query rows
    const size_t exact = (size_t)2 * kMWaves * 32 * kMKeyStride;               // exact phase: distance bits + indices
    if (img < qstage) img = qstage;
    if (img < exact) img = exact;
    img = (img + 3) & ~(size_t)3;
    p.img = (int)img;
    p.lds = img * 4 + fixed;
    // the exact phase's candidates pass through the tail (everything behind `small`); the allocation may grow up to the limit for it
    const size_t head = img * 4 + small, room = kMLdsMax - head;
    // staged exact phase: stages of 2^srl rows of 4D + 16 bytes (at most 8 stages, at most 8 sweeps of the block per stage).
    // 0 = gather from L2.
    const int DS = DP > 64 && D > 64 ? 64 : D;  // staged width of a row: D > 64 goes through in two column halves
    const int PR = DS / 4;
    const bool stageable = D % 4 == 0 && (kMThreads % PR) == 0 && aligned16;
    if (stageable) {
        for (int l = 8; l >= 5; --l) {
            const size_t need = ((size_t)1 << l) * ((size_t)DS * 4 + 16);
            if (need <= room && ((size_t)1 << l) * PR <= 8 * (size_t)kMThreads && ((M + (1 << l) - 1) >> l) <= 8) {
                p.srl = l;
                if (head + need > p.lds) p.lds = head + need;
                break;
            }
        }
    }
    // column slices instead of row stages: every row of the cloud, 16 dimensions at a time, as four planes of 16-byte
    // pieces -- when the whole cloud's slice fits the same tail (M <= 1024 at the kernel's 512 threads x 8 pieces)
    if (stageable && D % 16 == 0 && D <= 64 && M <= 8 * (kMThreads / 4)) {
        const size_t mpc = (size_t)(M + kMThreads / 4 - 1) / (kMThreads / 4) * (kMThreads / 4);
        const size_t need = 4 * (mpc * 16 + 32);
        if (need <= room) {
            p.csl = D / 16;  // (D <= 64, above: knn_mfma_kernel<4, ...> does not contain the column-slice code)
            p.srl = 0;  // (the decode does not group the ids by row stage)
            if (head + need > p.lds) p.lds = head + need;
        }
    }
    return p;
}

using KnnMfmaKernel = void (*)(KnnMfmaArgs);
using KnnPreImageKernel = void (*)(const float *, int, int, int, KnnPre);

// what the pre-pass kernels and knn_mfma_kernel<F16Pre> rely on besides D % 4 == 0: 16-byte loads of every row of x and y
bool knn_mfma_aligned16(const float *x, const float *y) { return ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(x)) & 15) == 0; }

}  // namespace

namespace fx3d {

size_t knn_mfma_pre_bytes(int M, int B, int D) { return KnnPre::make(nullptr, M, knn_mfma_dp(D)).stride * (size_t)B; }
bool knn_mfma_pre_shape_ok(int M, int D, int kk) {
    return D >= 4 && D <= 128 && kk <= 32 && M >= 64 && M <= 4096 && D % 4 == 0 && kPreThreads % (D / 4) == 0 && D / 4 <= 32;
}
// the shapes fx3d_knn_ws serves with the pre-pass: the fp16 filter (the default of knn_mfma_kernel)
bool knn_mfma_pre_eligible(const float *x, const float *y, int M, int D, int kk) {
    return knn_mfma_pre_shape_ok(M, D, kk) && knn_mfma_aligned16(x, y) && !(opt(OPT_KNN_NO_MFMA) || opt(OPT_KNN_NO_PREPASS));
}

fx3d_status knn_mfma_launch(const float *x, int N, const float *y, int M, int B, int D, int k, int drop, int32_t *idx, float *dist,
                            hipStream_t st, void *pre_ws, int xdiv) {
    // fp16 filter: needs 16-byte loads (D % 4 == 0, aligned clouds) and all norms in LDS up front
    const bool f16 = D % 4 == 0 && M <= 4096 && ((reinterpret_cast<uintptr_t>(y) & 15) == 0) && ((size_t)M * D * 4) % 16 == 0;
    const bool aligned16 = knn_mfma_aligned16(x, y);
    // behind the pre-pass only with a workspace AND operands its kernels can read 16 bytes at a time: x as well as y (every cloud
    // of the batch then: N * D * 4 and M * D * 4 are multiples of 16).  Otherwise the plain fp16 kernel, which stages any x through LDS.
    const bool use_pre = pre_ws != nullptr && f16 && aligned16;
    const int DP = knn_mfma_dp(D), di = DP / 64;  // DK = 1, 2, 4 -> 0, 1, 2
    static const KnnMfmaKernel kernels[3][3] = {
        {knn_mfma_kernel<1, KnnFilter::F32>, knn_mfma_kernel<1, KnnFilter::F16>, knn_mfma_kernel<1, KnnFilter::F16Pre>},
        {knn_mfma_kernel<2, KnnFilter::F32>, knn_mfma_kernel<2, KnnFilter::F16>, knn_mfma_kernel<2, KnnFilter::F16Pre>},
        {knn_mfma_kernel<4, KnnFilter::F32>, knn_mfma_kernel<4, KnnFilter::F16>, knn_mfma_kernel<4, KnnFilter::F16Pre>}};
    static const KnnPreImageKernel pre_image[3] = {knn_pre_image_kernel<1>, knn_pre_image_kernel<2>, knn_pre_image_kernel<4>};
    const KnnMfmaKernel kernel = kernels[di][use_pre ? 2 : (f16 ? 1 : 0)];
    const KnnMfmaPlan p = knn_mfma_plan(DP, f16, use_pre, M, D, aligned16);
    const fx3d_status arc = ensure_dynamic_lds(reinterpret_cast<const void *>(kernel), (int)kMLdsMax, use_pre ? "knn_mfma_kernel<pre>" : "knn_mfma_kernel");
    if (arc != FX3D_OK) return arc;
    FX3D_REQUIRE(p.lds <= kMLdsMax, "fx3d_knn: internal LDS plan exceeds the CU (D=%d)", D);
    FX3D_REQUIRE(p.csl == 0 || DP <= 64, "fx3d_knn: internal plan selects column slices at D=%d, which its kernel does not contain", D);
    const int qpb = kMWaves * 32;
    const int nbx = (N + qpb - 1) / qpb;
    const int bpad = B >= 8 ? (B + 7) / 8 * 8 : B;
    if (use_pre) {
        const KnnPre pre = KnnPre::make(pre_ws, M, DP);
        // (the batch in x with the parts, like the search kernel's: grid y stops at 65535 clouds)
        hipLaunchKernelGGL(knn_pre_stats_kernel, dim3(kPreParts * (unsigned int)B), dim3(kPreThreads), 0, st, y, M, D, DP, pre);
        hipLaunchKernelGGL(pre_image[di], dim3(kPreParts * (unsigned int)B), dim3(kPreThreads), 0, st, y, M, D, p.two_norms, pre);
    }
    const KnnMfmaArgs args{x, N, y, M, B, D, k, drop, idx, dist, p.CH, p.img, p.keep_norms, p.two_norms, p.srl, p.csl, use_pre ? pre_ws : nullptr, xdiv};
    hipLaunchKernelGGL(kernel, dim3(nbx * bpad), dim3(kMThreads), p.lds, st, args);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

}  // namespace fx3d
