/* flux3d_hip_layers.h -- the models' building blocks as layers in their own right, beside include/flux3d_hip.h (which this
 * header includes: status codes, fx3d_stream_t, fx3d_last_error, the allocation and copy entry points).  The functions are
 * exported by the same libflux3d_hip.so.  Everything flux3d_hip.h says about pointers (device unless named *_host), streams,
 * status codes and the thread-local error message holds here. */
#ifndef FLUX3D_HIP_LAYERS_H
#define FLUX3D_HIP_LAYERS_H

#include "flux3d_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- stnKD(K): the spatial-transformer block (src/models/pointnet.jl:3-20), test mode ------------------------------------------
 * The reference's other exported building block (src/models/pointnet.jl:1 exports stnKD and PointNet): PointNet's stn is
 * stnKD(3), its fstn stnKD(64); a cloud with normals takes stnKD(6).  Float32, BatchNorm at its running statistics.
 * x (K,N,B) device, channels first like every model of this library: point n of cloud b has channels x[:,n,b] (the reference's
 * Chain takes the permuted (N,K,B)).  1 <= K <= 128: one (64 x 130) LDS image holds the tile's input channels (EdgeConv's F has
 * the same limit).  In the order the layers run:
 *   conv K->64, relu, BN . conv 64->128, relu, BN . conv 128->1024, relu, BN . max over the N points (= pooled (1024,B)) .
 *   dense 1024->512, relu . dense 512->256, relu . BN(256) . dense 256->K K = d;
 *   out (K,K,B), out[i,j,b] = d[j + K i] (the reshape is column-major, then the transpose; no identity is added: the reference
 *   has its `x .+ I` commented out) -- the orientation of fx3d_pointnet_forward's stn and fstn.
 * Arithmetic: "PointNet inference"'s contract (flux3d_hip.h), verbatim -- one accumulator per output element,
 *   acc = fmaf(x[c], W[c,o], acc) for c ascending from +0.0f over ALL K input channels; one Float32 bias addition, then the
 *   epilogue in the layer's order with eps = 1f-5 and every operation rounded; relu and the maximum are Julia's max (NaN wins,
 *   max(-0.0, +0.0) = +0.0).  No contraction is split over waves or blocks and none is padded with zero channels (0 * Inf is
 *   NaN: an Inf weight next to a pad would change the result), no float atomics: out and pooled are bit-identical to the
 *   restatement tests/stnkd_ref.py and from run to run, and depend on (K, N, B) alone, never on the launch shape.  The first
 *   convolution runs on v_mfma_f32_32x32x2_f32 over the first 4 floor(K / 4) channels and goes on as v_fma_f32 on the same
 *   accumulators ("EdgeConv inference"'s first-layer rule; K < 4: v_fma_f32 alone).
 * params_dev: ONE flat device Float32 buffer, 4-byte aligned, the layers' arrays in forward order, each layer laid out as for
 *   PointNet (conv W (Cin,Cout) column-major then b; BatchNorm gamma, beta, mu, var; dense W (out,in) column-major then b):
 *   conv1, bn1, conv2, bn2, conv3, bn3, dense1, dense2, bn4, dense3.  That is the stn.* (K = 3) and the fstn.* (K = 64) slice of
 *   fx3d_pointnet_forward's buffer.  fx3d_stnkd_param_count(K) is its length in floats.
 * out (K,K,B) is required; pooled (1024,B) is optional (NULL: not written).  Refusals, before any device work, the message
 *   (fx3d_last_error) naming the value: K outside [1, 128] FX3D_ERR_UNSUPPORTED; FX3D_ERR_INVALID_ARG for N < 1, B < 1,
 *   B > 65535, N B > 2^31, a NULL required pointer, a short workspace or one not 16-byte aligned.
 * Two launches on `s` (three with pooled), no host synchronisation, no host memory read after the argument check
 * (Capture: fx3d_stnkd_forward: replayed).  ws: fx3d_stnkd_workspace_bytes(N, B, K) -- the per-tile maxima (1024,ntiles,B) --,
 * 16-byte aligned. */
#define FX3D_STNKD_MAX_K 128
FX3D_API fx3d_status fx3d_stnkd_param_count(int32_t K, int64_t *count);
/* Batch axis: fx3d_stnkd_workspace_bytes, fx3d_stnkd_forward: B <= 65535 -- the point kernel has the cloud on the grid's y;
 * refused by the size check, the query included, with a message that names B. */
FX3D_API fx3d_status fx3d_stnkd_workspace_bytes(int32_t N, int32_t B, int32_t K, size_t *bytes);
FX3D_API fx3d_status fx3d_stnkd_forward(const float *params_dev, int32_t K, const float *x, int32_t N, int32_t B, float *out,
                                        float *pooled, void *ws, size_t ws_bytes, fx3d_stream_t s);

/* ---- stnKD(K), training-mode forward: Flux's BatchNorm in training mode (stnKD has no Dropout) ---------------------------------
 * The layers, the layouts and all arithmetic but BatchNorm's statistics are "stnKD(K)" above.  Each of the four BatchNorms
 * normalises by the mean and the uncorrected variance of what it is given over the current batch -- relu(conv + bias), m = N B
 * values per channel, for bn1, bn2, bn3; relu(dense2 + bias), m = B, for bn4 -- and the running statistics Flux would then hold
 * are returned.  Sums, mean and variance, running update: "PointNet training-mode forward"'s (flux3d_hip.h), word for word:
 * Float64 S1 = sum v and S2 = sum v v per (channel, tile of 64 points) in two chains by bit 2 of the row, the tile sums
 * t = tile + ntiles b folded as FX3D_POINTNET_STAT_GROUPS interleaved chains; a dense BatchNorm one chain over the clouds in
 * ascending b; mu64 = S1 / m, var64 = max(0, S2 / m - mu64 mu64), each rounded to Float32 once; the running update in Float32
 * with mtm = momentum.  The orders depend on (N, B) alone; no atomics.
 * Statistics layout (batch_stats and running, FX3D_STNKD_STAT_COUNT floats): bn1, bn2, bn3, bn4 in that order, each mu (C) then
 *   var (C), C = 64, 128, 1024, 256.
 * out (required) and pooled (optional) as in fx3d_stnkd_forward; batch_stats is required; running is optional and is computed
 * from the mu / var slots of params_dev, which is not written.  out, pooled, batch_stats and running are bit-identical to the
 * restatement tests/stnkd_ref.py and from run to run.  fx3d_stnkd_forward on parameters whose mu / var slots hold batch_stats
 * gives the same out and pooled bit for bit; with the stn.* / fstn.* slice of a PointNet buffer and that network's x / h, out,
 * the statistics and the running values are fx3d_pointnet_forward_train's stn / fstn and their slots.
 * Refusals, before any device work: fx3d_stnkd_forward's; FX3D_ERR_INVALID_ARG for B < 2 (the dense BatchNorm's running
 * variance divides by B - 1) and for a momentum not finite or outside [0, 1].
 * 10 launches on `s` (11 with pooled), no host synchronisation, no host memory read after the argument check
 * (Capture: fx3d_stnkd_forward_train: replayed).  ws: fx3d_stnkd_train_workspace_bytes(N, B, K) -- the forward's workspace,
 * the tile sums (2,1024,ntiles,B) Float64 and the head's (256,B) activations --, 16-byte aligned. */
#define FX3D_STNKD_STAT_COUNT 2944 /* 2 (64 + 128 + 1024 + 256) */
/* Batch axis: fx3d_stnkd_train_workspace_bytes, fx3d_stnkd_forward_train: B <= 65535 -- as fx3d_stnkd_forward. */
FX3D_API fx3d_status fx3d_stnkd_train_workspace_bytes(int32_t N, int32_t B, int32_t K, size_t *bytes);
FX3D_API fx3d_status fx3d_stnkd_forward_train(const float *params_dev, int32_t K, const float *x, int32_t N, int32_t B,
                                              float momentum, float *out, float *pooled, float *batch_stats, float *running,
                                              void *ws, size_t ws_bytes, fx3d_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* FLUX3D_HIP_LAYERS_H */
