// PointCloud and TriMesh transforms (gfx950): scale, translate, rotate, and normalize / realign with their per-cloud or
// per-mesh statistics (src/transforms/pcloud_func.jl, src/transforms/mesh_func.jl:99-399).  include/flux3d_hip.h states the
// definitions; this file is how they are computed.
//
// Segments.  Every input is a (D, ncols) column-major float stream cut into B segments of whole columns: dense (D, N, B) has
// segment b = columns [b N, (b+1) N); packed (3, sum V) has segment b = columns [seg_off[b], seg_off[b+1]) with the int64 prefix
// sums on the device.  Either way segment b is the contiguous element range [D start_b, D end_b) and element i lies in row
// i % D, so one set of kernels serves both layouts.
//
// Plan (a function of D, n_max = the longest segment, and B only; fx3d_transform_plan_describe prints it): a chunk is
// kChunkFloats / D columns.  nchunks = ceil(n_max / chunk).  nchunks <= 1: FUSED, one block per segment computes the statistics
// and applies the map in one launch.  Otherwise TWO LAUNCHES: a (nchunks, B) grid writes one partial per (chunk, segment, row) to
// the caller's workspace, then a (nchunks, B) grid folds its segment's partials in a fixed order and maps its chunk.  No atomics,
// no inter-block hand-off, no host synchronisation.
//
// Statistics.  normalize: per chunk k of n_k points, sum_k = sum x (Float64) and M2_k = sum (x - m_k)^2 about m_k = sum_k / n_k
// (Float64).  The fold: S = sum_k sum_k, c = Float32(S / n), and sum (x - c)^2 = sum_k (M2_k + n_k (m_k - c)^2) (exact in exact
// arithmetic, and cancellation-free in Float64 for data far from the origin), s = Float32(sqrt(that / (n - 1))).  The block
// reductions, the chunk fold included, are the fixed tree of block_sum.  realign: Julia's min / max
// (NaN wins, -0 < +0), which are associative and commutative, so any order gives the same bits.
// Arithmetic of the maps follows the reference's broadcasts expression by expression, unfused (-ffp-contract=off).
#include <cmath>

#include "fx3d_common.h"

using namespace fx3d;

namespace {

constexpr int kThreads = 512;              // statistics and segment maps
constexpr int kFlatThreads = 256;          // flat maps (scale / translate / rotate)
constexpr int kFlatMaxBlocks = 8192;
constexpr long long kChunkFloats = 16384;  // floats per statistics chunk (64 KiB)
constexpr int kMaxD = 1024;                // rows of normalize / realign (per-row constants live in LDS)
constexpr float kEps = 1e-6f;              // EPS = Float32(1e-6) (src/transforms/utils.jl:4)

struct Mat9 { float r[9]; };               // one (3, 3) rotmat, column-major, by value
struct Vec3 { float v[3]; };               // a scale factor (v[0]) or a translation vector, by value

// Julia's min / max on IEEE floats (base/math.jl): NaN propagates, -0.0 < +0.0.  fminf / fmaxf do neither.
__device__ __forceinline__ float jmin(float x, float y) {
    return ((y < x) || (signbit(y) && !signbit(x))) ? (isnan(x) ? x : y) : (isnan(y) ? y : x);
}
__device__ __forceinline__ float jmax(float x, float y) {
    return ((y > x) || (!signbit(y) && signbit(x))) ? (isnan(x) ? x : y) : (isnan(y) ? y : x);
}

long long chunk_cols(int D) {
    const long long c = kChunkFloats / D;
    return c < 1 ? 1 : c;
}
long long num_chunks(int D, long long n_max) { return (n_max + chunk_cols(D) - 1) / chunk_cols(D); }

// columns [start, end) of segment b: dense when seg_off == nullptr
__device__ __forceinline__ void segment_cols(const int64_t *__restrict__ seg_off, long long n_max, int b, long long *start,
                                             long long *end) {
    if (seg_off) {
        *start = seg_off[b];
        *end = seg_off[b + 1];
    } else {
        *start = (long long)b * n_max;
        *end = *start + n_max;
    }
}

// the segment of column `col` (packed: binary search over seg_off[0..B])
__device__ __forceinline__ int segment_of(const int64_t *__restrict__ seg_off, long long n_max, int B, long long col) {
    if (!seg_off) return (int)(col / n_max);
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg_off[mid] <= col) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// --- block reductions (kThreads threads, fixed order) --------------------------------------------------------------------
__device__ __forceinline__ double block_sum_all(double v, double *red) {  // result in every thread
    const double r = block_sum<kThreads>(v, red);
    __syncthreads();
    if (threadIdx.x == 0) red[0] = r;
    __syncthreads();
    const double out = red[0];
    __syncthreads();
    return out;
}
template <bool MAX>
__device__ __forceinline__ float block_mm_all(float v, float *red) {  // Julia min / max over the block, result in every thread
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float o = __shfl_down(v, off, 64);
        v = MAX ? jmax(v, o) : jmin(v, o);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) red[w] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        float r = red[0];
        for (int i = 1; i < kThreads / 64; ++i) r = MAX ? jmax(r, red[i]) : jmin(r, red[i]);
        red[kThreads / 64] = r;
    }
    __syncthreads();
    const float out = red[kThreads / 64];
    __syncthreads();
    return out;
}

// (sum, M2 about the chunk mean) of row d over columns [c0, c1) -- two passes, the second from the cache
__device__ __forceinline__ void chunk_moments(const float *__restrict__ x, int D, int d, long long c0, long long c1, double *red,
                                              double *sum, double *m2) {
    double a = 0.0;
    for (long long j = c0 + threadIdx.x; j < c1; j += kThreads) a += (double)x[j * D + d];
    const double s = block_sum_all(a, red);
    const double m = s / (double)(c1 - c0);
    double q = 0.0;
    for (long long j = c0 + threadIdx.x; j < c1; j += kThreads) {
        const double t = (double)x[j * D + d] - m;
        q += t * t;
    }
    *sum = s;
    *m2 = block_sum_all(q, red);
}
__device__ __forceinline__ void chunk_minmax(const float *__restrict__ x, int D, int d, long long c0, long long c1, float *red,
                                             float *mn, float *mx) {
    float lo = __int_as_float(0x7f800000), hi = __int_as_float(0xff800000);  // +Inf / -Inf: neutral for Julia min / max
    for (long long j = c0 + threadIdx.x; j < c1; j += kThreads) {
        const float v = x[j * D + d];
        lo = jmin(lo, v);
        hi = jmax(hi, v);
    }
    *mn = block_mm_all<false>(lo, red);
    *mx = block_mm_all<true>(hi, red);
}

// c and s from the (sum_k, M2_k) of a segment's chunks 0..nk-1 (n_k from the chunk width and the segment length n)
__device__ __forceinline__ void fold_moments(const double2 *__restrict__ part, int D, int d, long long nk, long long cc, long long n,
                                             double *red, float *c, float *s) {
    double a = 0.0;
    for (long long k = threadIdx.x; k < nk; k += kThreads) a += part[k * D + d].x;
    const double S = block_sum_all(a, red);
    const float cf = (float)(S / (double)n);
    double q = 0.0;
    for (long long k = threadIdx.x; k < nk; k += kThreads) {
        const long long w = (n - k * cc) < cc ? (n - k * cc) : cc;
        const double2 p = part[k * D + d];
        const double mk = p.x / (double)w, t = mk - (double)cf;
        q += p.y + (double)w * (t * t);
    }
    const double Q = block_sum_all(q, red);
    *c = cf;
    *s = (float)sqrt(Q / (double)(n - 1));
}

// --- segment maps ---------------------------------------------------------------------------------------------------------
enum MapOp { MAP_NORM_ADD = 0, MAP_NORM_MAX = 1, MAP_REALIGN = 2 };

// y[i] = op(x[i]) over the element range [e0, e1) with per-row constants p0 / p1 / p2 / p3 (LDS): 16-byte loads and stores on
// the aligned middle, scalar head and tail.
template <int OP>
__device__ __forceinline__ float map_one(float v, int d, const float *p0, const float *p1, const float *p2, const float *p3) {
    if (OP == MAP_NORM_ADD) return (v - p0[d]) / p1[d];                 // p1 = s + EPS, computed once
    if (OP == MAP_NORM_MAX) return (v - p0[d]) / p1[d];                 // p1 = max(s, EPS), Julia's max
    return ((v - p0[d]) / p1[d]) * p2[d] + p3[d];                       // p0 smin, p1 (smax - smin) + EPS, p2 tmax - tmin, p3 tmin
}
template <int OP>
__device__ void map_range(const float *__restrict__ x, float *__restrict__ y, long long e0, long long e1, int D, const float *p0,
                          const float *p1, const float *p2, const float *p3) {
    long long a = (e0 + 3) & ~3ll;
    if (a > e1) a = e1;
    const long long bnd = a + ((e1 - a) & ~3ll);
    for (long long i = e0 + threadIdx.x; i < a; i += kThreads) y[i] = map_one<OP>(x[i], (int)(i % D), p0, p1, p2, p3);
    const int step = (int)((4ll * kThreads) % D);
    int d = (int)((a + 4ll * threadIdx.x) % D);
    for (long long i = a + 4ll * threadIdx.x; i < bnd; i += 4ll * kThreads) {
        const float4 v = *reinterpret_cast<const float4 *>(x + i);
        const int d1 = d + 1 == D ? 0 : d + 1, d2 = d1 + 1 == D ? 0 : d1 + 1, d3 = d2 + 1 == D ? 0 : d2 + 1;
        float4 o;
        o.x = map_one<OP>(v.x, d, p0, p1, p2, p3);
        o.y = map_one<OP>(v.y, d1, p0, p1, p2, p3);
        o.z = map_one<OP>(v.z, d2, p0, p1, p2, p3);
        o.w = map_one<OP>(v.w, d3, p0, p1, p2, p3);
        *reinterpret_cast<float4 *>(y + i) = o;
        d += step;
        if (d >= D) d -= D;
    }
    for (long long i = bnd + threadIdx.x; i < e1; i += kThreads) y[i] = map_one<OP>(x[i], (int)(i % D), p0, p1, p2, p3);
}

// --- kernels --------------------------------------------------------------------------------------------------------------
// Per-chunk partials, grid (nchunks, B): MINMAX writes float2 (min, max), otherwise double2 (sum, M2), at [(b nchunks + k) D + d].
template <bool MINMAX>
__global__ __launch_bounds__(kThreads) void seg_partials_kernel(const float *__restrict__ x, int D, long long n_max,
                                                                const int64_t *__restrict__ seg_off, long long cc, void *part) {
    __shared__ double red[kThreads / 64 + 1];
    const int k = blockIdx.x, b = blockIdx.y;
    long long st, en;
    segment_cols(seg_off, n_max, b, &st, &en);
    const long long c0 = st + (long long)k * cc;
    if (c0 >= en) return;  // a chunk past this segment's end: never read by the fold
    const long long c1 = c0 + cc < en ? c0 + cc : en;
    const long long slot = ((long long)b * gridDim.x + k) * D;
    for (int d = 0; d < D; ++d) {
        if (MINMAX) {
            float mn, mx;
            chunk_minmax(x, D, d, c0, c1, reinterpret_cast<float *>(red), &mn, &mx);
            if (threadIdx.x == 0) static_cast<float2 *>(part)[slot + d] = make_float2(mn, mx);
        } else {
            double s, q;
            chunk_moments(x, D, d, c0, c1, red, &s, &q);
            if (threadIdx.x == 0) static_cast<double2 *>(part)[slot + d] = make_double2(s, q);
        }
    }
}

// Min / max per (row, segment) into mn / mx (D, B).  part == nullptr: FUSED, the block reduces its whole segment; otherwise it
// folds the segment's partials.  pad_zero: a segment shorter than n_max also folds in +0.0 (realign! over verts_padded).
// Grid B.  An empty segment gives +Inf / -Inf (the host rejects empty realign inputs before any launch).
__global__ __launch_bounds__(kThreads) void seg_minmax_kernel(const float *__restrict__ x, int D, long long n_max,
                                                              const int64_t *__restrict__ seg_off, const float2 *__restrict__ part,
                                                              long long nchunks, long long cc, int pad_zero, float *__restrict__ mn,
                                                              float *__restrict__ mx) {
    __shared__ float red[kThreads / 64 + 1];
    const int b = blockIdx.x;
    long long st, en;
    segment_cols(seg_off, n_max, b, &st, &en);
    const long long nk = (en - st + cc - 1) / cc;
    for (int d = 0; d < D; ++d) {
        float lo, hi;
        if (!part) {
            chunk_minmax(x, D, d, st, en, red, &lo, &hi);
        } else {
            float l = __int_as_float(0x7f800000), h = __int_as_float(0xff800000);
            for (long long k = threadIdx.x; k < nk; k += kThreads) {
                const float2 p = part[((long long)b * nchunks + k) * D + d];
                l = jmin(l, p.x);
                h = jmax(h, p.y);
            }
            lo = block_mm_all<false>(l, red);
            hi = block_mm_all<true>(h, red);
        }
        if (pad_zero && en - st < n_max) {
            lo = jmin(lo, 0.0f);
            hi = jmax(hi, 0.0f);
        }
        if (threadIdx.x == 0) {
            mn[(long long)b * D + d] = lo;
            mx[(long long)b * D + d] = hi;
        }
    }
}

// normalize, grid (nchunks, B): the block's segment statistics (FUSED: from its one chunk; else folded from the partials),
// then the map of chunk blockIdx.x.  Block (0, b) writes centroid / scale (D, B) when asked.
template <int OP>
__global__ __launch_bounds__(kThreads) void normalize_kernel(const float *__restrict__ x, int D, long long n_max,
                                                             const int64_t *__restrict__ seg_off, const double2 *__restrict__ part,
                                                             long long cc, float *__restrict__ y, float *__restrict__ cout,
                                                             float *__restrict__ sout) {
    __shared__ double red[kThreads / 64 + 1];
    __shared__ float pc[kMaxD], ps[kMaxD];
    const int k = blockIdx.x, b = blockIdx.y;
    long long st, en;
    segment_cols(seg_off, n_max, b, &st, &en);
    const long long n = en - st;
    const long long c0 = st + (long long)k * cc;
    if (c0 >= en && !(k == 0 && (cout || sout))) return;
    const long long nk = (n + cc - 1) / cc;
    for (int d = 0; d < D; ++d) {
        float c, s;
        if (!part) {
            double sm = 0.0, q = 0.0;
            if (n > 0) chunk_moments(x, D, d, st, en, red, &sm, &q);
            // the fold of one partial
            c = (float)(sm / (double)n);
            const double t = (n > 0 ? sm / (double)n : 0.0) - (double)c;
            s = (float)sqrt((q + (double)n * (t * t)) / (double)(n - 1));
        } else {
            fold_moments(part + (long long)b * gridDim.x * D, D, d, nk, cc, n, red, &c, &s);
        }
        if (threadIdx.x == 0) {
            pc[d] = c;
            ps[d] = OP == MAP_NORM_ADD ? s + kEps : jmax(s, kEps);
            if (k == 0 && cout) cout[(long long)b * D + d] = c;
            if (k == 0 && sout) sout[(long long)b * D + d] = s;
        }
    }
    __syncthreads();
    if (c0 >= en) return;
    const long long c1 = c0 + cc < en ? c0 + cc : en;
    map_range<OP>(x, y, c0 * D, c1 * D, D, pc, ps, nullptr, nullptr);
}

// realign's map, grid (nchunks, B): y = ((x - smin) / ((smax - smin) + EPS)) * (tmax - tmin) + tmin per (row, segment)
__global__ __launch_bounds__(kThreads) void realign_kernel(const float *__restrict__ x, int D, long long n_max,
                                                           const int64_t *__restrict__ seg_off, long long cc,
                                                           const float *__restrict__ smin, const float *__restrict__ smax,
                                                           const float *__restrict__ tmin, const float *__restrict__ tmax,
                                                           float *__restrict__ y) {
    __shared__ float p0[kMaxD], p1[kMaxD], p2[kMaxD], p3[kMaxD];
    const int k = blockIdx.x, b = blockIdx.y;
    long long st, en;
    segment_cols(seg_off, n_max, b, &st, &en);
    const long long c0 = st + (long long)k * cc;
    if (c0 >= en) return;
    for (int d = threadIdx.x; d < D; d += kThreads) {
        const float lo = smin[(long long)b * D + d], hi = smax[(long long)b * D + d];
        p0[d] = lo;
        p1[d] = (hi - lo) + kEps;
        p2[d] = tmax[d] - tmin[d];
        p3[d] = tmin[d];
    }
    __syncthreads();
    const long long c1 = c0 + cc < en ? c0 + cc : en;
    map_range<MAP_REALIGN>(x, y, c0 * D, c1 * D, D, p0, p1, p2, p3);
}

// scale (factor * x) or translate (x + t[i % 3]) over a flat stream of n floats: 16-byte loads and stores, grid-stride
template <bool TRANSLATE>
__global__ __launch_bounds__(kFlatThreads) void affine_kernel(const float *__restrict__ x, long long n, Vec3 a, float *__restrict__ y) {
    const long long n4 = n >> 2, stride = (long long)gridDim.x * kFlatThreads;
    for (long long q = (long long)blockIdx.x * kFlatThreads + threadIdx.x; q < n4; q += stride) {
        const float4 v = *reinterpret_cast<const float4 *>(x + 4 * q);
        float4 o;
        if (TRANSLATE) {
            const int d = (int)((4 * q) % 3);
            const int d1 = d == 2 ? 0 : d + 1, d2 = d1 == 2 ? 0 : d1 + 1;
            o.x = v.x + a.v[d]; o.y = v.y + a.v[d1]; o.z = v.z + a.v[d2]; o.w = v.w + a.v[d];
        } else {
            o.x = a.v[0] * v.x; o.y = a.v[0] * v.y; o.z = a.v[0] * v.z; o.w = a.v[0] * v.w;
        }
        *reinterpret_cast<float4 *>(y + 4 * q) = o;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const long long i = 4 * n4 + threadIdx.x;
        y[i] = TRANSLATE ? x[i] + a.v[i % 3] : a.v[0] * x[i];
    }
}

// y[:, j] = transpose(R) * x[:, j]: y_i = (R[0,i] x0 + R[1,i] x1) + R[2,i] x2.  Four columns (48 bytes, three 16-byte loads)
// per thread and step.  rdev != nullptr: R of column j's segment from (3, 3, B), else the by-value matrix.
__device__ __forceinline__ void rot_col(const float *r, float x0, float x1, float x2, float *o) {
    o[0] = ((r[0] * x0) + (r[1] * x1)) + (r[2] * x2);
    o[1] = ((r[3] * x0) + (r[4] * x1)) + (r[5] * x2);
    o[2] = ((r[6] * x0) + (r[7] * x1)) + (r[8] * x2);
}
__global__ __launch_bounds__(kFlatThreads) void rotate_kernel(const float *__restrict__ x, long long ncols, long long n_max, int B,
                                                              const int64_t *__restrict__ seg_off, Mat9 m,
                                                              const float *__restrict__ rdev, float *__restrict__ y) {
    const long long nq = ncols >> 2, stride = (long long)gridDim.x * kFlatThreads;
    for (long long q = (long long)blockIdx.x * kFlatThreads + threadIdx.x; q < nq; q += stride) {
        const float4 *xp = reinterpret_cast<const float4 *>(x + 12 * q);
        const float4 a = xp[0], b = xp[1], c = xp[2];
        const float in[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
        float out[12];
        long long seg = -1, seg_end = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float r[9];
            if (rdev) {
                const long long col = 4 * q + u;
                if (seg < 0 || col >= seg_end) {
                    seg = segment_of(seg_off, n_max, B, col);
                    seg_end = seg_off ? seg_off[seg + 1] : (seg + 1) * n_max;
                }
#pragma unroll
                for (int e = 0; e < 9; ++e) r[e] = rdev[9 * seg + e];
            } else {
#pragma unroll
                for (int e = 0; e < 9; ++e) r[e] = m.r[e];
            }
            rot_col(r, in[3 * u], in[3 * u + 1], in[3 * u + 2], out + 3 * u);
        }
        float4 *yp = reinterpret_cast<float4 *>(y + 12 * q);
        yp[0] = make_float4(out[0], out[1], out[2], out[3]);
        yp[1] = make_float4(out[4], out[5], out[6], out[7]);
        yp[2] = make_float4(out[8], out[9], out[10], out[11]);
    }
    if (blockIdx.x == 0 && threadIdx.x < (ncols & 3)) {
        const long long col = 4 * nq + threadIdx.x;
        float r[9];
        const long long seg = rdev ? segment_of(seg_off, n_max, B, col) : 0;
        for (int e = 0; e < 9; ++e) r[e] = rdev ? rdev[9 * seg + e] : m.r[e];
        float o[3];
        rot_col(r, x[3 * col], x[3 * col + 1], x[3 * col + 2], o);
        y[3 * col] = o[0]; y[3 * col + 1] = o[1]; y[3 * col + 2] = o[2];
    }
}

int flat_grid(long long work) {
    long long g = (work + kFlatThreads - 1) / kFlatThreads;
    if (g > kFlatMaxBlocks) g = kFlatMaxBlocks;
    return (int)(g < 1 ? 1 : g);
}

fx3d_status check_segments(const char *fn, int D, long long n_max, int B, int max_d) {
    FX3D_REQUIRE(D >= 1 && D <= max_d, "%s: D = %d outside [1, %d]", fn, D, max_d);
    FX3D_REQUIRE(B >= 1 && B <= 65535, "%s: B = %d outside [1, 65535]", fn, B);
    FX3D_REQUIRE(n_max >= 0 && n_max < (1ll << 40), "%s: bad n_max = %lld", fn, n_max);
    FX3D_REQUIRE(num_chunks(D, n_max) < (1ll << 31), "%s: too many chunks", fn);
    return FX3D_OK;
}

size_t ws_need(int D, long long n_max, int B) {
    const long long nk = num_chunks(D, n_max);
    if (nk <= 1) return 0;
    return (size_t)nk * B * D * sizeof(double2);
}

fx3d_status check_ws(const char *fn, int D, long long n_max, int B, const void *ws, size_t ws_bytes) {
    const size_t need = ws_need(D, n_max, B);
    if (need && (!ws || ws_bytes < need)) {
        set_error("%s: workspace too small (%zu < %zu)", fn, ws_bytes, need);
        return FX3D_ERR_WORKSPACE;
    }
    return FX3D_OK;
}

}  // namespace

extern "C" {

fx3d_status fx3d_transform_plan_describe(int32_t D, int64_t n_max, int32_t B, char *buf, size_t len) {
    FX3D_REQUIRE(buf && len > 0, "fx3d_transform_plan_describe: null buffer");
    fx3d_status rc = check_segments("fx3d_transform_plan_describe", D, n_max, B, 1 << 30);
    if (rc) return rc;
    const long long nk = num_chunks(D, n_max);
    snprintf(buf, len, "plan=%s chunk_cols=%lld nchunks=%lld grid=%lldx%d threads=%d ws=%zu", nk <= 1 ? "fused" : "two_launch",
             chunk_cols(D), nk, nk < 1 ? 1 : nk, B, kThreads, ws_need(D, n_max, B));
    return FX3D_OK;
}

fx3d_status fx3d_transform_workspace_bytes(int32_t D, int64_t n_max, int32_t B, size_t *bytes) {
    FX3D_REQUIRE(bytes, "fx3d_transform_workspace_bytes: null output");
    fx3d_status rc = check_segments("fx3d_transform_workspace_bytes", D, n_max, B, 1 << 30);
    if (rc) return rc;
    *bytes = ws_need(D, n_max, B);
    return FX3D_OK;
}

fx3d_status fx3d_segment_minmax(const float *x, int32_t D, int64_t n_max, int32_t B, const int64_t *seg_off, int32_t pad_zero,
                                float *min_out, float *max_out, void *ws, size_t ws_bytes, fx3d_stream_t s) {
    FX3D_REQUIRE(x && min_out && max_out, "fx3d_segment_minmax: null pointer");
    fx3d_status rc = check_segments("fx3d_segment_minmax", D, n_max, B, kMaxD);
    if (rc) return rc;
    FX3D_REQUIRE(n_max > 0, "fx3d_segment_minmax: reducing over an empty collection is not allowed");
    if ((rc = check_ws("fx3d_segment_minmax", D, n_max, B, ws, ws_bytes))) return rc;
    hipStream_t st = as_stream(s);
    const long long nk = num_chunks(D, n_max), cc = chunk_cols(D);
    ProfileScope prof("segment_minmax", st);
    if (nk > 1) {
        hipLaunchKernelGGL(seg_partials_kernel<true>, dim3((unsigned)nk, B), dim3(kThreads), 0, st, x, (int)D, (long long)n_max,
                           seg_off, cc, ws);
        FX3D_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(seg_minmax_kernel, dim3(B), dim3(kThreads), 0, st, x, (int)D, (long long)n_max, seg_off,
                       nk > 1 ? static_cast<const float2 *>(ws) : nullptr, nk, cc, (int)(pad_zero != 0), min_out, max_out);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

fx3d_status fx3d_normalize(const float *x, int32_t D, int64_t n_max, int32_t B, const int64_t *seg_off, int32_t mode, float *y,
                           float *centroid_out, float *scale_out, void *ws, size_t ws_bytes, fx3d_stream_t s) {
    FX3D_REQUIRE(x && y, "fx3d_normalize: null pointer");
    FX3D_REQUIRE(mode == FX3D_NORMALIZE_EPS_ADD || mode == FX3D_NORMALIZE_EPS_MAX, "fx3d_normalize: bad mode %d", mode);
    fx3d_status rc = check_segments("fx3d_normalize", D, n_max, B, kMaxD);
    if (rc) return rc;
    if ((rc = check_ws("fx3d_normalize", D, n_max, B, ws, ws_bytes))) return rc;
    if (n_max == 0 && !centroid_out && !scale_out) return FX3D_OK;  // nothing to map, nothing asked
    hipStream_t st = as_stream(s);
    const long long nk = num_chunks(D, n_max), cc = chunk_cols(D);
    const dim3 grid((unsigned)(nk < 1 ? 1 : nk), B);
    ProfileScope prof("normalize", st);
    if (nk > 1) {
        hipLaunchKernelGGL(seg_partials_kernel<false>, grid, dim3(kThreads), 0, st, x, (int)D, (long long)n_max, seg_off, cc, ws);
        FX3D_LAUNCH_CHECK();
    }
    const double2 *part = nk > 1 ? static_cast<const double2 *>(ws) : nullptr;
    if (mode == FX3D_NORMALIZE_EPS_ADD)
        hipLaunchKernelGGL(normalize_kernel<MAP_NORM_ADD>, grid, dim3(kThreads), 0, st, x, (int)D, (long long)n_max, seg_off, part,
                           cc, y, centroid_out, scale_out);
    else
        hipLaunchKernelGGL(normalize_kernel<MAP_NORM_MAX>, grid, dim3(kThreads), 0, st, x, (int)D, (long long)n_max, seg_off, part,
                           cc, y, centroid_out, scale_out);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

fx3d_status fx3d_realign(const float *x, int32_t D, int64_t n_max, int32_t B, const int64_t *seg_off, const float *src_min,
                         const float *src_max, const float *tgt_min, const float *tgt_max, float *y, fx3d_stream_t s) {
    FX3D_REQUIRE(x && y && src_min && src_max && tgt_min && tgt_max, "fx3d_realign: null pointer");
    fx3d_status rc = check_segments("fx3d_realign", D, n_max, B, kMaxD);
    if (rc) return rc;
    if (n_max == 0) return FX3D_OK;
    hipStream_t st = as_stream(s);
    const long long nk = num_chunks(D, n_max), cc = chunk_cols(D);
    ProfileScope prof("realign", st);
    hipLaunchKernelGGL(realign_kernel, dim3((unsigned)nk, B), dim3(kThreads), 0, st, x, (int)D, (long long)n_max, seg_off, cc,
                       src_min, src_max, tgt_min, tgt_max, y);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

fx3d_status fx3d_rotate(const float *x, int64_t ncols, int64_t n_max, int32_t B, const int64_t *seg_off, const float *rotmat_host,
                        const float *rotmat_dev, float *y, fx3d_stream_t s) {
    FX3D_REQUIRE(x && y, "fx3d_rotate: null pointer");
    FX3D_REQUIRE((rotmat_host != nullptr) != (rotmat_dev != nullptr), "fx3d_rotate: pass exactly one of rotmat_host, rotmat_dev");
    fx3d_status rc = check_segments("fx3d_rotate", 3, n_max, B, 3);
    if (rc) return rc;
    FX3D_REQUIRE(ncols >= 0 && ncols < (1ll << 40), "fx3d_rotate: bad ncols = %lld", (long long)ncols);
    FX3D_REQUIRE(seg_off || ncols == n_max * B, "fx3d_rotate: dense input needs ncols == n_max * B");
    Mat9 m{};
    if (rotmat_host)
        for (int e = 0; e < 9; ++e) m.r[e] = rotmat_host[e];
    if (ncols == 0) return FX3D_OK;
    hipStream_t st = as_stream(s);
    ProfileScope prof("rotate", st);
    hipLaunchKernelGGL(rotate_kernel, dim3(flat_grid((ncols + 3) / 4)), dim3(kFlatThreads), 0, st, x, (long long)ncols,
                       (long long)n_max, (int)B, seg_off, m, rotmat_dev, y);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

fx3d_status fx3d_scale_translate(const float *x, int64_t n, int32_t mode, const float *vec_host, float *y, fx3d_stream_t s) {
    FX3D_REQUIRE(x && y && vec_host, "fx3d_scale_translate: null pointer");
    FX3D_REQUIRE(mode == FX3D_SCALE || mode == FX3D_TRANSLATE, "fx3d_scale_translate: bad mode %d", mode);
    FX3D_REQUIRE(n >= 0 && n < (1ll << 42), "fx3d_scale_translate: bad n = %lld", (long long)n);
    FX3D_REQUIRE(mode == FX3D_SCALE || n % 3 == 0, "fx3d_scale_translate: translate needs D = 3 (n %% 3 == 0)");
    Vec3 a{};
    a.v[0] = vec_host[0];
    if (mode == FX3D_TRANSLATE) { a.v[1] = vec_host[1]; a.v[2] = vec_host[2]; }
    if (n == 0) return FX3D_OK;
    hipStream_t st = as_stream(s);
    ProfileScope prof(mode == FX3D_SCALE ? "scale" : "translate", st);
    if (mode == FX3D_SCALE)
        hipLaunchKernelGGL(affine_kernel<false>, dim3(flat_grid((n + 3) / 4)), dim3(kFlatThreads), 0, st, x, (long long)n, a, y);
    else
        hipLaunchKernelGGL(affine_kernel<true>, dim3(flat_grid((n + 3) / 4)), dim3(kFlatThreads), 0, st, x, (long long)n, a, y);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

}  // extern "C"
