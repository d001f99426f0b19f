// The training step around forward_train / grad_train (gfx950): include/flux3d_hip.h "Training step".  fx3d_crossentropy (loss,
// glogits and the accuracy count from probs), fx3d_dropout_mask (Dropout(p)'s multipliers drawn on the device) and fx3d_adam_step
// (Flux.Optimise.ADAM over one flat buffer, the running statistics written into the parameters).  Small or streaming kernels; the
// header states their arithmetic, tests/train_step_ref.py restates it.
#include <algorithm>
#include <cmath>

#include "fx3d_common.h"
#include "philox.h"

using namespace fx3d;

namespace {

constexpr int kThreads = 256;
constexpr int kAdamMaxBlocks = 2048;  // 8 blocks per CU; the rest of a larger buffer by grid stride

// One block.  Part 1, all threads over the (num_classes, B) elements: glogits.  Part 2, columns in chunks of kThreads: thread t takes
// column b = chunk + t (its term of the loss, its first maximum, its label's check), thread 0 then adds the chunk's terms to the one
// chain in ascending b and counts.
__global__ __launch_bounds__(kThreads) void crossentropy_kernel(const float *__restrict__ probs, const int32_t *__restrict__ labels,
                                                               int nc, int B, float *__restrict__ glogits, double *__restrict__ loss,
                                                               int32_t *__restrict__ counts) {
    __shared__ double term[kThreads];
    __shared__ int flag[kThreads];  // bit 0: the first maximum is the label; bit 1: the label is out of range
    const int tid = threadIdx.x;
    const float fB = (float)B;
    const long long total = (long long)nc * B;
    for (long long e = tid; e < total; e += kThreads) {
        const int b = (int)(e / nc), o = (int)(e % nc);
        const float hot = (o == labels[b]) ? 1.0f : 0.0f;  // (a label out of range matches no row)
        glogits[e] = (probs[e] - hot) / fB;
    }
    double sum = 0.0;
    int correct = 0, bad = 0;
    for (int b0 = 0; b0 < B; b0 += kThreads) {
        const int b = b0 + tid;
        if (b < B) {
            const float *col = probs + (size_t)b * nc;
            const int y = labels[b];
            int best = 0;
            float pbest = col[0];
            for (int o = 1; o < nc; ++o) {
                const float p = col[o];
                if (p > pbest) { pbest = p; best = o; }
            }
            const bool in = y >= 0 && y < nc;
            term[tid] = in ? log((double)col[y]) : (double)NAN;
            flag[tid] = in ? (best == y ? 1 : 0) : 2;
        }
        __syncthreads();
        if (tid == 0) {
            const int cnt = min(kThreads, B - b0);
            for (int i = 0; i < cnt; ++i) {
                sum = sum + term[i];
                correct += flag[i] & 1;
                bad += flag[i] >> 1;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        *loss = (-sum) / (double)B;
        counts[0] = correct;
        counts[1] = bad;
    }
}

// Thread t: one Philox block, elements 4 t .. 4 t + 3.
__global__ __launch_bounds__(kThreads) void dropout_mask_kernel(long long n, double p, float keep, uint64_t seed_host,
                                                               const uint64_t *__restrict__ counter_dev, uint32_t stream_id,
                                                               float *__restrict__ out) {
    const uint64_t seed = seed_host + (counter_dev ? *counter_dev : 0);  // (sample_seeded_kernel's convention)
    const long long nq = (n + 3) / 4;
    const bool vec = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    for (long long q = (long long)blockIdx.x * kThreads + threadIdx.x; q < nq; q += (long long)gridDim.x * kThreads) {
        uint32_t c[4] = {(uint32_t)q, stream_id, 0u, 0u};
        philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
        float w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float u = (float)(c[j] >> 8) * (1.0f / 16777216.0f);
            w[j] = ((double)u > p) ? keep : 0.0f;
        }
        const long long e = 4 * q;
        if (vec && e + 4 <= n) {
            *reinterpret_cast<float4 *>(out + e) = float4{w[0], w[1], w[2], w[3]};
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (e + j < n) out[e + j] = w[j];
        }
    }
}

struct AdamHyper {
    double eta, beta1, beta2, eps;
};

// One element of Flux.Optimise.ADAM, the header's four lines; den1 = 1 - betap[0], den2 = 1 - betap[1], omb = 1 - beta.
__device__ __forceinline__ void adam_element(const AdamHyper &h, double omb1, double omb2, double den1, double den2, float g, float &m,
                                             float &v, float &x) {
    m = (float)((h.beta1 * (double)m) + (omb1 * (double)g));
    const float gg = g * g;
    v = (float)((h.beta2 * (double)v) + (omb2 * (double)gg));
    const float delta = (float)((((double)m / den1) / (sqrt((double)v / den2) + h.eps)) * h.eta);
    x = x - delta;
}

// VEC: the four pointers reach 16 bytes after the same `head` elements.  Elements [0, head) and [head + 4 nvec, n) one per thread of
// block 0, the nvec groups of four between them as float4 by grid stride.  Otherwise one element per thread by grid stride.  betap
// is only read here.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void adam_kernel(long long n, int head, long long nvec, AdamHyper h, const float *__restrict__ g,
                                                       float *__restrict__ m, float *__restrict__ v,
                                                       const double *__restrict__ betap, float *__restrict__ x) {
    const double omb1 = 1.0 - h.beta1, omb2 = 1.0 - h.beta2;
    const double den1 = 1.0 - betap[0], den2 = 1.0 - betap[1];
    if (!VEC) {
        for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < n; e += (long long)gridDim.x * kThreads) {
            float mv = m[e], vv = v[e], xv = x[e];
            adam_element(h, omb1, omb2, den1, den2, g[e], mv, vv, xv);
            m[e] = mv; v[e] = vv; x[e] = xv;
        }
        return;
    }
    const float4 *g4 = reinterpret_cast<const float4 *>(g + head);
    float4 *m4 = reinterpret_cast<float4 *>(m + head), *v4 = reinterpret_cast<float4 *>(v + head), *x4 = reinterpret_cast<float4 *>(x + head);
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < nvec; i += (long long)gridDim.x * kThreads) {
        const float4 gv = g4[i];
        float4 mv = m4[i], vv = v4[i], xv = x4[i];
        adam_element(h, omb1, omb2, den1, den2, gv.x, mv.x, vv.x, xv.x);
        adam_element(h, omb1, omb2, den1, den2, gv.y, mv.y, vv.y, xv.y);
        adam_element(h, omb1, omb2, den1, den2, gv.z, mv.z, vv.z, xv.z);
        adam_element(h, omb1, omb2, den1, den2, gv.w, mv.w, vv.w, xv.w);
        m4[i] = mv; v4[i] = vv; x4[i] = xv;
    }
    if (blockIdx.x == 0) {
        const long long body = head + 4 * nvec, rest = n - 4 * nvec;  // rest: head + tail elements
        for (long long r = threadIdx.x; r < rest; r += kThreads) {
            const long long e = r < head ? r : body + (r - head);
            float mv = m[e], vv = v[e], xv = x[e];
            adam_element(h, omb1, omb2, den1, den2, g[e], mv, vv, xv);
            m[e] = mv; v[e] = vv; x[e] = xv;
        }
    }
}

// After adam_kernel in stream order: the running statistics into their slots of x, and betap advanced by one step.
__global__ __launch_bounds__(kThreads) void adam_finish_kernel(long long n, double beta1, double beta2, double *__restrict__ betap,
                                                              float *__restrict__ x, const float *__restrict__ running,
                                                              const int32_t *__restrict__ stat_map, long long nstat) {
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < nstat; i += (long long)gridDim.x * kThreads) {
        const long long at = stat_map[i];
        if (at >= 0 && at < n) x[at] = running[i];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        betap[0] = betap[0] * beta1;
        betap[1] = betap[1] * beta2;
    }
}

}  // namespace

extern "C" {

fx3d_status fx3d_crossentropy(const float *probs, const int32_t *labels, int32_t num_classes, int32_t B, float *glogits, double *loss,
                              int32_t *counts, fx3d_stream_t s) {
    FX3D_REQUIRE(probs && labels && glogits && loss && counts, "fx3d_crossentropy: null pointer");
    FX3D_REQUIRE(num_classes >= 1 && B >= 1, "fx3d_crossentropy: need num_classes >= 1 and B >= 1, got %d, %d", num_classes, B);
    FX3D_REQUIRE((reinterpret_cast<uintptr_t>(loss) & 7) == 0, "fx3d_crossentropy: loss must be 8-byte aligned");
    FX3D_REQUIRE_DEVICE();
    hipLaunchKernelGGL(crossentropy_kernel, dim3(1), dim3(kThreads), 0, as_stream(s), probs, labels, (int)num_classes, (int)B, glogits,
                       loss, counts);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

fx3d_status fx3d_dropout_mask(int64_t n, double p, uint64_t seed, const uint64_t *counter_dev, int32_t stream_id, float *out,
                              fx3d_stream_t s) {
    FX3D_REQUIRE(out, "fx3d_dropout_mask: null pointer");
    FX3D_REQUIRE(n >= 0 && n <= ((int64_t)1 << 34), "fx3d_dropout_mask: n must be in [0, 2^34], got %lld", (long long)n);
    FX3D_REQUIRE(p >= 0.0 && p < 1.0, "fx3d_dropout_mask: p must be in [0, 1), got %g", p);
    FX3D_REQUIRE(stream_id >= 0, "fx3d_dropout_mask: stream_id must not be negative, got %d", stream_id);
    FX3D_REQUIRE((reinterpret_cast<uintptr_t>(counter_dev) & 7) == 0, "fx3d_dropout_mask: counter_dev must be 8-byte aligned");
    if (n == 0) return FX3D_OK;
    FX3D_REQUIRE_DEVICE();
    const long long nq = (n + 3) / 4;
    const long long grid = std::min<long long>((nq + kThreads - 1) / kThreads, kAdamMaxBlocks);
    hipLaunchKernelGGL(dropout_mask_kernel, dim3((unsigned)grid), dim3(kThreads), 0, as_stream(s), (long long)n, p,
                       (float)(1.0 / (1.0 - p)), seed, counter_dev, (uint32_t)stream_id, out);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

fx3d_status fx3d_adam_step(int64_t n, double eta, double beta1, double beta2, double eps, const float *g, float *m, float *v,
                           double *betap, float *x, const float *running, const int32_t *stat_map, int64_t nstat, fx3d_stream_t s) {
    FX3D_REQUIRE(n >= 0 && nstat >= 0, "fx3d_adam_step: n and nstat must not be negative, got %lld, %lld", (long long)n, (long long)nstat);
    FX3D_REQUIRE(g && m && v && betap && x, "fx3d_adam_step: null pointer");
    FX3D_REQUIRE(nstat == 0 || (running && stat_map), "fx3d_adam_step: nstat > 0 needs running and stat_map");
    FX3D_REQUIRE((reinterpret_cast<uintptr_t>(betap) & 7) == 0, "fx3d_adam_step: betap must be 8-byte aligned");
    FX3D_REQUIRE_DEVICE();
    const hipStream_t st = as_stream(s);
    if (n > 0) {
        // the float4 body needs one head for all four arrays
        const uintptr_t a = reinterpret_cast<uintptr_t>(x) & 15;
        const bool share = (reinterpret_cast<uintptr_t>(g) & 15) == a && (reinterpret_cast<uintptr_t>(m) & 15) == a &&
                           (reinterpret_cast<uintptr_t>(v) & 15) == a;
        const int head = (int)std::min<int64_t>(n, (int64_t)((16 - a) & 15) / 4);
        const long long nvec = (n - head) / 4;
        const long long work = share ? nvec : (long long)n;
        const long long grid = std::max<long long>(1, std::min<long long>((work + kThreads - 1) / kThreads, kAdamMaxBlocks));
        const AdamHyper h{eta, beta1, beta2, eps};
        if (share)
            hipLaunchKernelGGL(adam_kernel<true>, dim3((unsigned)grid), dim3(kThreads), 0, st, (long long)n, head, nvec, h, g, m, v, betap, x);
        else
            hipLaunchKernelGGL(adam_kernel<false>, dim3((unsigned)grid), dim3(kThreads), 0, st, (long long)n, 0, 0LL, h, g, m, v, betap, x);
        FX3D_LAUNCH_CHECK();
    }
    const long long fgrid = std::max<long long>(1, std::min<long long>((nstat + kThreads - 1) / kThreads, kAdamMaxBlocks));
    hipLaunchKernelGGL(adam_finish_kernel, dim3((unsigned)fgrid), dim3(kThreads), 0, st, (long long)n, beta1, beta2, betap, x, running,
                       stat_map, (long long)nstat);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

}  // extern "C"
