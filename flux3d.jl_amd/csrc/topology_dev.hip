// Mesh topology built on the device: the edge list and faces_to_edges (_compute_edges_packed, src/rep/mesh.jl:907-955), the
// uniform Laplacian in CSR (_compute_laplacian_packed, :957-1002), the vertex -> (face, corner) tables of the ordered sampling
// adjoint and the normals, and faces_padded -> faces_packed (_compute_faces_packed, :884-896).  Every output is bit for bit what
// the host builders of topology.cpp write from the same faces: those stay the comparator.
//
// One tool does all the ordering: a stable LSD radix sort of 64-bit elements, 8 bits per pass, that only visits the bit
// windows its caller knows to be occupied.
//   hist     a wave owns a tile of kTileKeys consecutive elements and counts its digits: hist[digit][tile] (digit-major)
//   scan     exclusive prefix sum of that array: the first output slot of (digit, tile), three launches (scan_exclusive)
//   scatter  the wave walks its tile again, 64 elements a round in input order.  The lanes holding one digit find each other
//            with 8 ballots; an element's slot = the tile's running slot of that digit + the number of lower lanes with the
//            same digit.  So equal digits keep their input order: within a round by lane, between rounds and tiles by the scan.
// No atomic places anything and the only counters that use integer atomics are the bad-id counts (sums: order-free), so no
// output bit depends on scheduling, and there is no float atomic.  The cost does not depend on the valence of any vertex: a
// fan of F faces around one hub sorts like any other 3F elements.
//   edges      element = lo << 32 | hi of the 3F face sides (the order of (V+1)(lo+1) + (hi+1), :928-929); sorted on the windows
//              of hi, then lo; heads (element != predecessor) are flagged, scanned and compacted: E and the unique list.  emit
//              splits the unique list into the (E,2) columns and finds each side's edge id by binary search in it.
//   Laplacian  element = row << 32 | col of the 2E + V triples (e1,e2) (e2,e1) (v,v); sorted the same way.  deg(r) = (elements
//              of row r) - 1, by binary search of the row starts: both ends of every edge are there, a self-edge twice.  A run of m
//              equal elements is one CSR entry: off the diagonal m copies of 1/deg summed in sequence, on the diagonal the
//              m - 1 self-edge copies and then -1 -- the host's order (its sort is by (row, col, position), the diagonal last).
//   vertex tables  element = (b Vmax + v) << 32 | face * 4 + corner in (b, face, corner) order, padding faces under a sentinel
//              key behind every mesh; sorted on the key windows only, so the stable sort leaves each vertex's entries
//              ascending.  Row starts by binary search.
#include "fx3d_common.h"
#include "scan_common.h"

namespace fx3d {
namespace {

typedef unsigned long long u64;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kRadixBits = 8;
constexpr int kRadix = 1 << kRadixBits;
constexpr int kRounds = 16;                         // elements per lane of a sort tile
constexpr int kTileKeys = kWave * kRounds;          // a wave's tile
constexpr int kScanItems = 16;                      // values per thread of a scan chunk
constexpr int kScanChunk = kThreads * kScanItems;
constexpr int kScanThreads = 1024;
constexpr long long kMaxElems = (1ll << 31) - 1;    // positions and counts are uint32 / int32

// ---- exclusive scan of n uint32 in place: chunk sums, one block over the sums, chunks again -----------------------
__global__ __launch_bounds__(kThreads) void td_scan_sums_kernel(const uint32_t *__restrict__ data, long long n,
                                                                uint32_t *__restrict__ sums) {
    __shared__ uint32_t sw[kWaves];
    const long long base = (long long)blockIdx.x * kScanChunk;
    uint32_t s = 0;
#pragma unroll
    for (int r = 0; r < kScanItems; ++r) {
        const long long i = base + r * kThreads + threadIdx.x;
        if (i < n) s += data[i];
    }
    for (int o = kWave / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0) sw[threadIdx.x / kWave] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int i = 0; i < kWaves; ++i) t += sw[i];
        sums[blockIdx.x] = t;
    }
}

// one block: sums -> their exclusive scan; the grand total into total_a / total_b (each optional)
__global__ __launch_bounds__(kScanThreads) void td_scan_top_kernel(uint32_t *__restrict__ sums, long long nb,
                                                                   int64_t *__restrict__ total_a,
                                                                   int64_t *__restrict__ total_b) {
    __shared__ uint32_t sw[kScanThreads / kWave];
    const uint32_t total = scan_entries<uint32_t, kScanThreads>(nb, [&](long long e) { return sums[e]; }, sums, sw);
    if (threadIdx.x == 0) {
        if (total_a) *total_a = (int64_t)total;
        if (total_b) *total_b = (int64_t)total;
    }
}

__global__ __launch_bounds__(kThreads) void td_scan_apply_kernel(uint32_t *__restrict__ data, long long n,
                                                                 const uint32_t *__restrict__ sums) {
    __shared__ uint32_t sw[kWaves];
    const long long base = (long long)blockIdx.x * kScanChunk;
    uint32_t carry = sums[blockIdx.x];
    for (int r = 0; r < kScanItems; ++r) {
        const long long i = base + r * kThreads + threadIdx.x;
        uint32_t tot;
        const uint32_t ex = block_exclusive_scan<uint32_t>(i < n ? data[i] : 0u, sw, &tot);
        if (i < n) data[i] = carry + ex;
        carry += tot;
    }
}

long long scan_chunks(long long n) { return (n + kScanChunk - 1) / kScanChunk; }

// data (n) in place; sums: scan_chunks(n) uint32 of scratch
void scan_exclusive(uint32_t *data, long long n, uint32_t *sums, int64_t *total_a, int64_t *total_b, hipStream_t st) {
    const long long nb = scan_chunks(n);
    hipLaunchKernelGGL(td_scan_sums_kernel, dim3((unsigned)nb), dim3(kThreads), 0, st, data, n, sums);
    hipLaunchKernelGGL(td_scan_top_kernel, dim3(1), dim3(kScanThreads), 0, st, sums, nb, total_a, total_b);
    hipLaunchKernelGGL(td_scan_apply_kernel, dim3((unsigned)nb), dim3(kThreads), 0, st, data, n, sums);
}

// ---- stable LSD radix sort ------------------------------------------------------------------------------------
// the lanes of the wave that are valid and hold digit d
__device__ __forceinline__ u64 digit_peers(unsigned d, bool valid) {
    u64 m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < kRadixBits; ++b) {
        const bool bit = (d >> b) & 1u;
        const u64 bal = __ballot(bit);
        m &= bit ? bal : ~bal;
    }
    return m;
}

__global__ __launch_bounds__(kThreads) void td_sort_hist_kernel(const u64 *__restrict__ in, long long n, int shift,
                                                                long long ntiles, uint32_t *__restrict__ hist) {
    __shared__ uint32_t cnt[kWaves][kRadix];
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    const long long tile = (long long)blockIdx.x * kWaves + w;
    for (int d = lane; d < kRadix; d += kWave) cnt[w][d] = 0;
    __syncthreads();
    for (int r = 0; r < kRounds; ++r) {  // (every wave runs every round: the barriers are block-wide)
        const long long i = tile * kTileKeys + r * kWave + lane;
        const bool valid = tile < ntiles && i < n;
        const unsigned d = valid ? (unsigned)(in[i] >> shift) & (kRadix - 1) : 0u;
        const u64 peers = digit_peers(d, valid);
        const bool lead = valid && (peers & ((1ull << lane) - 1)) == 0;  // one lane per digit present: no two touch a counter
        if (lead) cnt[w][d] += (uint32_t)__popcll(peers);
        __syncthreads();
    }
    if (tile < ntiles)
        for (int d = lane; d < kRadix; d += kWave) hist[(long long)d * ntiles + tile] = cnt[w][d];
}

__global__ __launch_bounds__(kThreads) void td_sort_scatter_kernel(const u64 *__restrict__ in, u64 *__restrict__ out,
                                                                   long long n, int shift, long long ntiles,
                                                                   const uint32_t *__restrict__ offs) {
    __shared__ uint32_t pos[kWaves][kRadix];  // the tile's next slot of every digit
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    const long long tile = (long long)blockIdx.x * kWaves + w;
    if (tile < ntiles)
        for (int d = lane; d < kRadix; d += kWave) pos[w][d] = offs[(long long)d * ntiles + tile];
    __syncthreads();
    for (int r = 0; r < kRounds; ++r) {
        const long long i = tile * kTileKeys + r * kWave + lane;
        const bool valid = tile < ntiles && i < n;
        const u64 key = valid ? in[i] : 0ull;
        const unsigned d = (unsigned)(key >> shift) & (kRadix - 1);
        const u64 peers = digit_peers(d, valid);
        const int rank = __popcll(peers & ((1ull << lane) - 1));
        const uint32_t p = valid ? pos[w][d] : 0u;
        __syncthreads();
        if (valid && rank == 0) pos[w][d] = p + (uint32_t)__popcll(peers);
        __syncthreads();
        if (valid) out[(long long)p + rank] = key;  // p + rank < n: the scan of the counts of these very elements
    }
}

long long sort_tiles(long long n) { return (n + kTileKeys - 1) / kTileKeys; }
int bits_for(u64 maxval) { return maxval == 0 ? 0 : 64 - __builtin_clzll(maxval); }

// the windows of a sort: bits [0, lo_bits) and [32, 32 + hi_bits), 8 at a time from the least significant
int sort_passes(int lo_bits, int hi_bits) { return (lo_bits + kRadixBits - 1) / kRadixBits + (hi_bits + kRadixBits - 1) / kRadixBits; }

// Sorts a (n elements) through b; returns the buffer that holds the result (a for an even number of passes).
// hist: kRadix * sort_tiles(n) uint32; sums: scan_chunks(kRadix * sort_tiles(n)) uint32.
u64 *radix_sort(u64 *a, u64 *b, long long n, int lo_bits, int hi_bits, uint32_t *hist, uint32_t *sums, hipStream_t st) {
    const long long ntiles = sort_tiles(n);
    const unsigned blocks = (unsigned)((ntiles + kWaves - 1) / kWaves);
    for (int half = 0; half < 2; ++half) {
        const int from = half ? 32 : 0, bits = half ? hi_bits : lo_bits;
        for (int shift = from; shift < from + bits; shift += kRadixBits) {
            hipLaunchKernelGGL(td_sort_hist_kernel, dim3(blocks), dim3(kThreads), 0, st, a, n, shift, ntiles, hist);
            scan_exclusive(hist, (long long)kRadix * ntiles, sums, nullptr, nullptr, st);
            hipLaunchKernelGGL(td_sort_scatter_kernel, dim3(blocks), dim3(kThreads), 0, st, a, b, n, shift, ntiles, hist);
            u64 *t = a;
            a = b;
            b = t;
        }
    }
    return a;
}

unsigned grid_for(long long n) {  // grid-stride element-wise launches
    const long long want = (n + kThreads - 1) / kThreads, cap = 32ll * device_cus();
    return (unsigned)(want < 1 ? 1 : want < cap ? want : cap);
}
#define TD_FOR(i, n) \
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < (n); i += (long long)gridDim.x * kThreads)

// first position of sorted[0, n) that is >= key
__device__ __forceinline__ long long lower_bound(const u64 *__restrict__ sorted, long long n, u64 key) {
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (sorted[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// flag[i] = 1 at the first element of every run of equal elements
__global__ __launch_bounds__(kThreads) void td_heads_kernel(const u64 *__restrict__ sorted, long long n,
                                                            uint32_t *__restrict__ flag) {
    TD_FOR(i, n) flag[i] = (i == 0 || sorted[i] != sorted[i - 1]) ? 1u : 0u;
}

// a wave's sum of per-lane counts into a device counter (an integer sum: the order of arrival changes nothing)
__device__ __forceinline__ void count_bad(uint32_t nbad, uint32_t *bad) {
    for (int o = kWave / 2; o > 0; o >>= 1) nbad += __shfl_xor(nbad, o, kWave);
    if (nbad && bad && (threadIdx.x & (kWave - 1)) == 0) atomicAdd(bad, nbad);
}

// ---- edges ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 side_key(int a, int b) {
    return a < b ? ((u64)(uint32_t)a << 32) | (uint32_t)b : ((u64)(uint32_t)b << 32) | (uint32_t)a;
}
// the corner ids of face f, ids outside [0, V) replaced by 0 (never used as an index) and counted in *nbad
__device__ __forceinline__ void face_ids(const int32_t *__restrict__ faces, long long f, long long V, int v[3], uint32_t *nbad) {
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int x = faces[3 * f + t];
        const bool ok = x >= 0 && (long long)x < V;
        v[t] = ok ? x : 0;
        *nbad += ok ? 0u : 1u;
    }
}

// keys[e F + f], e = 0, 1, 2: the sides (v1,v2) (v2,v3) (v3,v1) of face f (:921-929)
__global__ __launch_bounds__(kThreads) void td_edge_keys_kernel(const int32_t *__restrict__ faces, long long F, long long V,
                                                                u64 *__restrict__ keys, uint32_t *__restrict__ bad) {
    const long long span = ((F + kThreads - 1) / kThreads) * kThreads;  // whole waves reach count_bad together
    TD_FOR(f, span) {
        uint32_t nbad = 0;
        if (f < F) {
            int v[3];
            face_ids(faces, f, V, v, &nbad);
            keys[f] = side_key(v[0], v[1]);
            keys[F + f] = side_key(v[1], v[2]);
            keys[2 * F + f] = side_key(v[2], v[0]);
        }
        count_bad(nbad, bad);
    }
}

__global__ __launch_bounds__(kThreads) void td_compact_kernel(const u64 *__restrict__ sorted, long long n,
                                                              const uint32_t *__restrict__ slot, u64 *__restrict__ uniq) {
    TD_FOR(i, n) if (i == 0 || sorted[i] != sorted[i - 1]) uniq[slot[i]] = sorted[i];
}

__global__ __launch_bounds__(kThreads) void td_edges_emit_kernel(const u64 *__restrict__ uniq, const int64_t *__restrict__ have,
                                                                 long long E, int32_t *__restrict__ edges) {
    const long long n = E < *have ? E : *have;  // never behind what count left, never behind the caller's E rows
    TD_FOR(e, n) {
        const u64 k = uniq[e];
        edges[e] = (int32_t)(k >> 32);
        edges[E + e] = (int32_t)(k & 0xffffffffull);
    }
}

// faces_to_edges (F,3) column-major, columns (e23, e31, e12) (:946): the position of each side in the unique list
__global__ __launch_bounds__(kThreads) void td_f2e_kernel(const int32_t *__restrict__ faces, long long F, long long V,
                                                          const u64 *__restrict__ uniq, const int64_t *__restrict__ have,
                                                          int32_t *__restrict__ f2e) {
    const long long E = *have;
    TD_FOR(f, F) {
        int v[3];
        uint32_t nbad = 0;
        face_ids(faces, f, V, v, &nbad);
        f2e[2 * F + f] = (int32_t)lower_bound(uniq, E, side_key(v[0], v[1]));
        f2e[f] = (int32_t)lower_bound(uniq, E, side_key(v[1], v[2]));
        f2e[F + f] = (int32_t)lower_bound(uniq, E, side_key(v[2], v[0]));
    }
}

// the buffers of one sort of n elements plus the flags of its runs
struct SortLayout {
    size_t a, b, hist, sums, flag, fsums, count, total;
};
SortLayout sort_layout(long long n) {
    const long long nh = (long long)kRadix * sort_tiles(n);
    WsBump ws;
    SortLayout l;
    l.a = ws.put(8 * (size_t)n);
    l.b = ws.put(8 * (size_t)n);
    l.hist = ws.put(4 * (size_t)nh);
    l.sums = ws.put(4 * (size_t)scan_chunks(nh));
    l.flag = ws.put(4 * (size_t)n);
    l.fsums = ws.put(4 * (size_t)scan_chunks(n));
    l.count = ws.put(8);
    l.total = ws.at;
    return l;
}

bool edge_sizes_ok(int64_t F, int64_t V) { return F > 0 && V > 0 && F <= kMaxElems / 3 && V <= kMaxElems; }
bool lap_sizes_ok(int64_t E, int64_t V) { return E >= 0 && V > 0 && E <= kMaxElems && V <= kMaxElems && 2 * E + V <= kMaxElems; }
bool vf_sizes_ok(int32_t Vmax, int32_t Fmax, int32_t B) {
    return Vmax > 0 && Fmax > 0 && B > 0 && Fmax < (1 << 29) && 3ll * Fmax * B <= kMaxElems && (long long)Vmax * B < kMaxElems;
}

// ---- Laplacian --------------------------------------------------------------------------------------------------
// the 2E + V triples as row << 32 | col: (e1,e2), (e2,e1), (v,v) (:976-997); ids outside [0, V) become 0 and are counted
__global__ __launch_bounds__(kThreads) void td_lap_keys_kernel(const int32_t *__restrict__ edges, long long E, long long V,
                                                               u64 *__restrict__ keys, uint32_t *__restrict__ bad) {
    const long long n = E + V, span = ((n + kThreads - 1) / kThreads) * kThreads;
    TD_FOR(t, span) {
        uint32_t nbad = 0;
        if (t < E) {
            int i = edges[t], j = edges[E + t];
            if (i < 0 || i >= V) { i = 0; ++nbad; }
            if (j < 0 || j >= V) { j = 0; ++nbad; }
            keys[t] = ((u64)(uint32_t)i << 32) | (uint32_t)j;
            keys[E + t] = ((u64)(uint32_t)j << 32) | (uint32_t)i;
        } else if (t < n) {
            const u64 v = (u64)(t - E);
            keys[2 * E + (t - E)] = (v << 32) | v;
        }
        count_bad(nbad, bad);
    }
}

// raw[r], r = 0..V: the first sorted triple of row r (raw[V] = n).  Row r holds both ends of its edges and its diagonal.
__global__ __launch_bounds__(kThreads) void td_lap_rows_kernel(const u64 *__restrict__ sorted, long long n, long long V,
                                                               uint32_t *__restrict__ raw) {
    TD_FOR(r, V + 1) raw[r] = (uint32_t)lower_bound(sorted, n, (u64)r << 32);
}

__global__ __launch_bounds__(kThreads) void td_lap_write_kernel(const u64 *__restrict__ sorted, long long n, long long V,
                                                                const uint32_t *__restrict__ raw,
                                                                const uint32_t *__restrict__ slot,
                                                                int32_t *__restrict__ rowptr, int32_t *__restrict__ colind,
                                                                float *__restrict__ vals) {
    TD_FOR(i, n) {
        const u64 k = sorted[i];
        if (i > 0 && sorted[i - 1] == k) continue;
        long long m = 1;  // equal triples: distinct edges give 1 off the diagonal and 1 or 3 on it
        while (i + m < n && sorted[i + m] == k) ++m;
        const long long r = (long long)(k >> 32), c = (long long)(k & 0xffffffffull);
        const long long deg = (long long)raw[r + 1] - (long long)raw[r] - 1;
        const float inv = deg > 0 ? (float)(1.0 / (double)deg) : (float)deg;  // (:986-988)
        float v;
        if (r != c) {
            v = inv;
            for (long long q = 1; q < m; ++q) v = v + inv;
        } else if (m == 1) {
            v = -1.0f;
        } else {  // the self-edge copies in the order of the triples, the diagonal's -1 last
            v = inv;
            for (long long q = 2; q < m; ++q) v = v + inv;
            v = v + -1.0f;
        }
        const uint32_t p = slot[i];
        colind[p] = (int32_t)c;
        vals[p] = v;
        if (raw[r] == (uint32_t)i) rowptr[r] = (int32_t)p;
    }
}

__global__ void td_lap_end_kernel(const int64_t *__restrict__ nnz, long long V, int32_t *__restrict__ rowptr) {
    rowptr[V] = (int32_t)*nnz;
}

struct LapLayout {
    SortLayout s;
    size_t raw, total;
};
LapLayout lap_layout(int64_t E, int64_t V) {
    LapLayout l;
    l.s = sort_layout(2 * E + V);
    WsBump ws{l.s.total};  // behind the sort's buffers
    l.raw = ws.put(4 * (size_t)(V + 1));
    l.total = ws.at;
    return l;
}

// ---- vertex -> (face, corner) tables ------------------------------------------------------------------------------
__device__ __forceinline__ int clamp_len(int L, int Fmax) { return L < 0 ? 0 : L > Fmax ? Fmax : L; }

// element (b Fmax + f) 3 + t = key << 32 | f * 4 + t, key = b Vmax + v, or B Vmax for what no table holds
__global__ __launch_bounds__(kThreads) void td_vf_keys_kernel(const int32_t *__restrict__ faces, const int32_t *__restrict__ faces_len,
                                                              int Vmax, int Fmax, int B, u64 *__restrict__ keys,
                                                              uint32_t *__restrict__ bad) {
    const long long n = (long long)Fmax * B, span = ((n + kThreads - 1) / kThreads) * kThreads;
    const u64 none = (u64)Vmax * (u64)B;
    TD_FOR(g, span) {
        uint32_t nbad = 0;
        if (g < n) {
            const int b = (int)(g / Fmax), f = (int)(g - (long long)b * Fmax);
            const int L = faces_len ? faces_len[b] : Fmax;
            if (f == 0 && (L < 0 || L > Fmax)) ++nbad;
            const bool live = f < clamp_len(L, Fmax);
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                u64 key = none;
                if (live) {
                    const int v = faces[3 * g + t];
                    if (v >= 0 && v < Vmax) key = (u64)b * (u64)Vmax + (u64)v;
                    else ++nbad;
                }
                keys[3 * g + t] = (key << 32) | (u64)(uint32_t)(f * 4 + t);
            }
        }
        count_bad(nbad, bad);
    }
}

// mstart[b], b = 0..B: the first sorted element of mesh b (mstart[B]: the first that belongs to no table)
__global__ __launch_bounds__(kThreads) void td_vf_starts_kernel(const u64 *__restrict__ sorted, long long n, int Vmax, int B,
                                                                uint32_t *__restrict__ mstart) {
    TD_FOR(b, (long long)B + 1) mstart[b] = (uint32_t)lower_bound(sorted, n, ((u64)b * (u64)Vmax) << 32);
}

__global__ __launch_bounds__(kThreads) void td_vf_rowptr_kernel(const u64 *__restrict__ sorted, long long n, int Vmax, int B,
                                                                const uint32_t *__restrict__ mstart,
                                                                int32_t *__restrict__ rowptr) {
    TD_FOR(g, (long long)(Vmax + 1) * B) {
        const long long b = g / (Vmax + 1), v = g - b * (Vmax + 1);
        const long long lb = v == 0 ? (long long)mstart[b] : v == Vmax ? (long long)mstart[b + 1]
                                                                      : lower_bound(sorted, n, ((u64)b * (u64)Vmax + (u64)v) << 32);
        rowptr[g] = (int32_t)(lb - (long long)mstart[b]);
    }
}

// the entries of mesh b fill the first vf_rowptr[Vmax, b] slots of its column; the rest are 0
__global__ __launch_bounds__(kThreads) void td_vf_ent_kernel(const u64 *__restrict__ sorted, int Fmax, int B,
                                                             const uint32_t *__restrict__ mstart, int32_t *__restrict__ ent) {
    TD_FOR(g, 3ll * Fmax * B) {
        const long long b = g / (3ll * Fmax), k = g - b * 3ll * Fmax;
        const long long s0 = mstart[b], cnt = (long long)mstart[b + 1] - s0;
        ent[g] = k < cnt ? (int32_t)(sorted[s0 + k] & 0xffffffffull) : 0;
    }
}

struct VfLayout {
    SortLayout s;
    size_t mstart, total;
};
VfLayout vf_layout(int32_t Fmax, int32_t B) {
    VfLayout l;
    l.s = sort_layout(3ll * Fmax * B);
    WsBump ws{l.s.total};  // behind the sort's buffers
    l.mstart = ws.put(4 * ((size_t)B + 1));
    l.total = ws.at;
    return l;
}

// ---- faces_padded -> faces_packed ----------------------------------------------------------------------------------
// one block: foff[b], voff[b], b = 0..B: faces / vertices of the meshes before b
__global__ __launch_bounds__(kScanThreads) void td_pack_offsets_kernel(const int32_t *__restrict__ faces_len,
                                                                       const int32_t *__restrict__ nverts, int Fmax, int B,
                                                                       long long *__restrict__ foff, long long *__restrict__ voff) {
    __shared__ long long sw[kScanThreads / kWave];
    const long long sumf = scan_entries<long long, kScanThreads>(
        B, [&](long long b) -> long long { return clamp_len(faces_len[b], Fmax); }, foff, sw);
    const long long sumv = scan_entries<long long, kScanThreads>(
        B, [&](long long b) -> long long { return nverts[b] > 0 ? nverts[b] : 0; }, voff, sw);
    if (threadIdx.x == 0) {
        foff[B] = sumf;
        voff[B] = sumv;
    }
}

__global__ __launch_bounds__(kThreads) void td_pack_faces_kernel(const int32_t *__restrict__ faces, int Fmax, int B,
                                                                 const long long *__restrict__ foff,
                                                                 const long long *__restrict__ voff, long long sumF,
                                                                 int32_t *__restrict__ out) {
    TD_FOR(g, 3ll * Fmax * B) {
        const long long b = g / (3ll * Fmax), e = g - b * 3ll * Fmax;
        const long long f0 = foff[b], f1 = foff[b + 1];
        if (e < 3 * (f1 - f0) && f1 <= sumF) out[3 * f0 + e] = (int32_t)((long long)faces[g] + voff[b]);
    }
}

struct PackLayout {
    size_t foff, voff, total;
};
PackLayout pack_layout(int32_t B) {
    WsBump ws;
    PackLayout l;
    l.foff = ws.put(8 * ((size_t)B + 1));
    l.voff = ws.put(8 * ((size_t)B + 1));
    l.total = ws.at;
    return l;
}

}  // namespace
}  // namespace fx3d

using namespace fx3d;

extern "C" {

fx3d_status fx3d_edges_dev_workspace_bytes(int64_t F, int64_t V, size_t *bytes) {
    FX3D_REQUIRE(bytes && edge_sizes_ok(F, V), "fx3d_edges_dev_workspace_bytes: bad arguments F=%lld V=%lld", (long long)F, (long long)V);
    *bytes = sort_layout(3 * F).total;
    return FX3D_OK;
}

fx3d_status fx3d_edges_dev_count(const int32_t *faces_packed, int64_t F, int64_t V, int64_t *E_dev, uint32_t *bad_dev,
                                 void *ws, size_t ws_bytes, fx3d_stream_t s) {
    FX3D_REQUIRE(edge_sizes_ok(F, V), "fx3d_edges_dev_count: bad sizes F=%lld V=%lld (F, V > 0, 3F < 2^31)", (long long)F, (long long)V);
    FX3D_REQUIRE(faces_packed && E_dev && bad_dev && ws, "fx3d_edges_dev_count: null pointer");
    const long long n = 3 * F;
    const SortLayout l = sort_layout(n);
    FX3D_REQUIRE(ws_bytes >= l.total, "fx3d_edges_dev_count: workspace too small");
    FX3D_REQUIRE_DEVICE();
    hipStream_t st = as_stream(s);
    char *w = static_cast<char *>(ws);
    auto *a = reinterpret_cast<u64 *>(w + l.a), *b = reinterpret_cast<u64 *>(w + l.b);
    auto *flag = reinterpret_cast<uint32_t *>(w + l.flag);
    FX3D_FILL(bad_dev, 0, sizeof(uint32_t), st);
    ProfileScope prof("edges_dev_count", st);
    hipLaunchKernelGGL(td_edge_keys_kernel, dim3(grid_for(F)), dim3(kThreads), 0, st, faces_packed, (long long)F, (long long)V, a, bad_dev);
    const int vb = bits_for((u64)V - 1);
    u64 *sorted = radix_sort(a, b, n, vb, vb, reinterpret_cast<uint32_t *>(w + l.hist), reinterpret_cast<uint32_t *>(w + l.sums), st);
    u64 *uniq = sorted == a ? b : a;
    hipLaunchKernelGGL(td_heads_kernel, dim3(grid_for(n)), dim3(kThreads), 0, st, sorted, n, flag);
    scan_exclusive(flag, n, reinterpret_cast<uint32_t *>(w + l.fsums), E_dev, reinterpret_cast<int64_t *>(w + l.count), st);
    hipLaunchKernelGGL(td_compact_kernel, dim3(grid_for(n)), dim3(kThreads), 0, st, sorted, n, flag, uniq);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

fx3d_status fx3d_edges_dev_emit(const int32_t *faces_packed, int64_t F, int64_t V, int64_t E, int32_t *edges,
                                int32_t *faces_to_edges, void *ws, size_t ws_bytes, fx3d_stream_t s) {
    FX3D_REQUIRE(edge_sizes_ok(F, V) && E > 0 && E <= 3 * F, "fx3d_edges_dev_emit: bad sizes F=%lld V=%lld E=%lld", (long long)F,
                 (long long)V, (long long)E);
    FX3D_REQUIRE(edges && ws && (faces_packed || !faces_to_edges), "fx3d_edges_dev_emit: null pointer");
    const SortLayout l = sort_layout(3 * F);
    FX3D_REQUIRE(ws_bytes >= l.total, "fx3d_edges_dev_emit: workspace too small");
    FX3D_REQUIRE_DEVICE();
    hipStream_t st = as_stream(s);
    char *w = static_cast<char *>(ws);
    const int vb = bits_for((u64)V - 1);
    // count left the sorted sides in a after an even number of passes, in b after an odd one, and the unique list in the other
    const u64 *uniq = reinterpret_cast<const u64 *>(w + (sort_passes(vb, vb) % 2 == 0 ? l.b : l.a));
    const int64_t *have = reinterpret_cast<const int64_t *>(w + l.count);
    ProfileScope prof("edges_dev_emit", st);
    hipLaunchKernelGGL(td_edges_emit_kernel, dim3(grid_for(E)), dim3(kThreads), 0, st, uniq, have, (long long)E, edges);
    if (faces_to_edges)
        hipLaunchKernelGGL(td_f2e_kernel, dim3(grid_for(F)), dim3(kThreads), 0, st, faces_packed, (long long)F, (long long)V, uniq, have,
                           faces_to_edges);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

fx3d_status fx3d_laplacian_dev_workspace_bytes(int64_t E, int64_t V, size_t *bytes) {
    FX3D_REQUIRE(bytes && lap_sizes_ok(E, V), "fx3d_laplacian_dev_workspace_bytes: bad arguments E=%lld V=%lld", (long long)E, (long long)V);
    *bytes = lap_layout(E, V).total;
    return FX3D_OK;
}

fx3d_status fx3d_laplacian_dev_csr(const int32_t *edges, int64_t E, int64_t V, int32_t *rowptr, int32_t *colind, float *vals,
                                   int64_t *nnz_dev, uint32_t *bad_dev, void *ws, size_t ws_bytes, fx3d_stream_t s) {
    FX3D_REQUIRE(lap_sizes_ok(E, V), "fx3d_laplacian_dev_csr: bad sizes E=%lld V=%lld (V > 0, 2E + V < 2^31)", (long long)E, (long long)V);
    FX3D_REQUIRE(edges && rowptr && colind && vals && nnz_dev && ws, "fx3d_laplacian_dev_csr: null pointer");
    const long long n = 2 * E + V;
    const LapLayout l = lap_layout(E, V);
    FX3D_REQUIRE(ws_bytes >= l.total, "fx3d_laplacian_dev_csr: workspace too small");
    FX3D_REQUIRE_DEVICE();
    hipStream_t st = as_stream(s);
    char *w = static_cast<char *>(ws);
    auto *a = reinterpret_cast<u64 *>(w + l.s.a), *b = reinterpret_cast<u64 *>(w + l.s.b);
    auto *flag = reinterpret_cast<uint32_t *>(w + l.s.flag), *raw = reinterpret_cast<uint32_t *>(w + l.raw);
    if (bad_dev) FX3D_FILL(bad_dev, 0, sizeof(uint32_t), st);
    ProfileScope prof("laplacian_dev_csr", st);
    hipLaunchKernelGGL(td_lap_keys_kernel, dim3(grid_for(E + V)), dim3(kThreads), 0, st, edges, (long long)E, (long long)V, a, bad_dev);
    const int vb = bits_for((u64)V - 1);
    const u64 *sorted = radix_sort(a, b, n, vb, vb, reinterpret_cast<uint32_t *>(w + l.s.hist), reinterpret_cast<uint32_t *>(w + l.s.sums), st);
    hipLaunchKernelGGL(td_lap_rows_kernel, dim3(grid_for(V + 1)), dim3(kThreads), 0, st, sorted, n, (long long)V, raw);
    hipLaunchKernelGGL(td_heads_kernel, dim3(grid_for(n)), dim3(kThreads), 0, st, sorted, n, flag);
    scan_exclusive(flag, n, reinterpret_cast<uint32_t *>(w + l.s.fsums), nnz_dev, nullptr, st);
    hipLaunchKernelGGL(td_lap_write_kernel, dim3(grid_for(n)), dim3(kThreads), 0, st, sorted, n, (long long)V, raw, flag, rowptr, colind, vals);
    hipLaunchKernelGGL(td_lap_end_kernel, dim3(1), dim3(1), 0, st, nnz_dev, (long long)V, rowptr);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

fx3d_status fx3d_vertex_faces_dev_workspace_bytes(int32_t Vmax, int32_t Fmax, int32_t B, size_t *bytes) {
    FX3D_REQUIRE(bytes && vf_sizes_ok(Vmax, Fmax, B), "fx3d_vertex_faces_dev_workspace_bytes: bad arguments Vmax=%d Fmax=%d B=%d", Vmax, Fmax, B);
    *bytes = vf_layout(Fmax, B).total;
    return FX3D_OK;
}

fx3d_status fx3d_vertex_faces_dev(const int32_t *faces_padded, const int32_t *faces_len, int32_t Vmax, int32_t Fmax, int32_t B,
                                  int32_t *vf_rowptr, int32_t *vf_ent, uint32_t *bad_dev, void *ws, size_t ws_bytes,
                                  fx3d_stream_t s) {
    FX3D_REQUIRE(vf_sizes_ok(Vmax, Fmax, B), "fx3d_vertex_faces_dev: bad sizes Vmax=%d Fmax=%d B=%d (Fmax < 2^29, 3 Fmax B < 2^31, Vmax B < 2^31)",
                 Vmax, Fmax, B);
    FX3D_REQUIRE(faces_padded && vf_rowptr && vf_ent && ws, "fx3d_vertex_faces_dev: null pointer");
    const long long n = 3ll * Fmax * B;
    const VfLayout l = vf_layout(Fmax, B);
    FX3D_REQUIRE(ws_bytes >= l.total, "fx3d_vertex_faces_dev: workspace too small");
    FX3D_REQUIRE_DEVICE();
    hipStream_t st = as_stream(s);
    char *w = static_cast<char *>(ws);
    auto *a = reinterpret_cast<u64 *>(w + l.s.a), *b = reinterpret_cast<u64 *>(w + l.s.b);
    auto *mstart = reinterpret_cast<uint32_t *>(w + l.mstart);
    if (bad_dev) FX3D_FILL(bad_dev, 0, sizeof(uint32_t), st);
    ProfileScope prof("vertex_faces_dev", st);
    hipLaunchKernelGGL(td_vf_keys_kernel, dim3(grid_for((long long)Fmax * B)), dim3(kThreads), 0, st, faces_padded, faces_len, Vmax, Fmax, B, a, bad_dev);
    const u64 *sorted = radix_sort(a, b, n, 0, bits_for((u64)Vmax * (u64)B), reinterpret_cast<uint32_t *>(w + l.s.hist),
                                   reinterpret_cast<uint32_t *>(w + l.s.sums), st);
    hipLaunchKernelGGL(td_vf_starts_kernel, dim3(grid_for((long long)B + 1)), dim3(kThreads), 0, st, sorted, n, Vmax, B, mstart);
    hipLaunchKernelGGL(td_vf_rowptr_kernel, dim3(grid_for((long long)(Vmax + 1) * B)), dim3(kThreads), 0, st, sorted, n, Vmax, B, mstart, vf_rowptr);
    hipLaunchKernelGGL(td_vf_ent_kernel, dim3(grid_for(n)), dim3(kThreads), 0, st, sorted, Fmax, B, mstart, vf_ent);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

fx3d_status fx3d_faces_padded_to_packed_dev_workspace_bytes(int32_t B, size_t *bytes) {
    FX3D_REQUIRE(bytes && B > 0, "fx3d_faces_padded_to_packed_dev_workspace_bytes: bad arguments B=%d", B);
    *bytes = pack_layout(B).total;
    return FX3D_OK;
}

fx3d_status fx3d_faces_padded_to_packed_dev(const int32_t *faces_padded, const int32_t *faces_len, const int32_t *nverts,
                                            int32_t Fmax, int32_t B, int64_t sumF, int32_t *faces_packed, void *ws,
                                            size_t ws_bytes, fx3d_stream_t s) {
    FX3D_REQUIRE(Fmax > 0 && B > 0 && Fmax < (1 << 29) && sumF > 0 && sumF <= (int64_t)Fmax * B,
                 "fx3d_faces_padded_to_packed_dev: bad sizes Fmax=%d B=%d sumF=%lld", Fmax, B, (long long)sumF);
    FX3D_REQUIRE(faces_padded && faces_len && nverts && faces_packed && ws, "fx3d_faces_padded_to_packed_dev: null pointer");
    const PackLayout l = pack_layout(B);
    FX3D_REQUIRE(ws_bytes >= l.total, "fx3d_faces_padded_to_packed_dev: workspace too small");
    FX3D_REQUIRE_DEVICE();
    hipStream_t st = as_stream(s);
    char *w = static_cast<char *>(ws);
    auto *foff = reinterpret_cast<long long *>(w + l.foff), *voff = reinterpret_cast<long long *>(w + l.voff);
    hipLaunchKernelGGL(td_pack_offsets_kernel, dim3(1), dim3(kScanThreads), 0, st, faces_len, nverts, Fmax, B, foff, voff);
    hipLaunchKernelGGL(td_pack_faces_kernel, dim3(grid_for(3ll * Fmax * B)), dim3(kThreads), 0, st, faces_padded, Fmax, B, foff, voff,
                       (long long)sumF, faces_packed);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

}  // extern "C"
