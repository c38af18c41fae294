// loss_scale.hip -- dynamic loss scaling of the fp16 training step, on the device and inside the two replayed graphs
// (include/sniper_hip.h: the layout of the eight doubles d_ls).
//   * the two loss-gradient kernels that inject the scale read it from d_ls[0] instead of taking it as a launch argument: the
//     statements are the ones of sn_softmax_output_bwd / the MakeLoss fill (softmax_grad.h), and a power-of-two scale commutes with
//     every rounding in them, so scale = S gives the bits of the plain kernels called with grad_scale * S;
//   * sn_grad_guard_scaled: the partial pass of sn_grad_guard (grad_guard.hip: the same kernel, grid and workspace) and a single-block
//     finalize that reports the norm in true units, puts 1 / S into the coefficient the guarded update multiplies with, and then
//     moves the scale: halve on a non-finite step, double after growth_interval clean ones (torch.cuda.amp.GradScaler's rule)
//     between min_scale and max_scale;
//   * sn_aux_shadow: the vectors the training forward writes as a side effect (BatchNorm moving statistics) saved before the forward
//     and put back after a skipped step, one launch for the whole table.
// No atomics: the same bits every run.
#include <math.h>

#include "common.h"
#include "grad_guard.h"
#include "softmax_grad.h"

namespace {

__global__ __launch_bounds__(256) void softmax_bwd_scaled_kernel(const float *__restrict__ p, const float *__restrict__ label,
                                                                 float *__restrict__ g, long outer, int K, long inner, float ignore,
                                                                 int use_ignore, float grad_scale, int normalize_valid,
                                                                 const int *__restrict__ valid_count, const double *__restrict__ ls) {
  const float scale = (float)ls[0];
  softmax_bwd_strided(p, label, g, outer, K, inner, ignore, use_ignore,
                      softmax_grad_mul(grad_scale * scale, normalize_valid, valid_count));
}

__global__ __launch_bounds__(256) void softmax_rows_bwd_scaled_kernel(const float *__restrict__ p, const float *__restrict__ label,
                                                                      float *__restrict__ g, long outer, int K, int R, SnDiv dK,
                                                                      float ignore, int use_ignore, float grad_scale,
                                                                      int normalize_valid, const int *__restrict__ valid_count,
                                                                      const double *__restrict__ ls) {
  const float scale = (float)ls[0];
  softmax_bwd_rows(p, label, g, outer, K, R, dK, ignore, use_ignore, softmax_grad_mul(grad_scale * scale, normalize_valid, valid_count));
}

__global__ __launch_bounds__(256) void fill_scaled_kernel(float *__restrict__ out, long n, float value, const double *__restrict__ ls) {
  const float v = value * (float)ls[0];
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) out[i] = v;
}

__global__ __launch_bounds__(kThreads) void grad_guard_scaled_finalize_kernel(const double *__restrict__ psum,
                                                                              const unsigned long long *__restrict__ pcnt, int nblk,
                                                                              const float *__restrict__ hyper, float clip_global_norm,
                                                                              int growth_interval, double growth_factor,
                                                                              double backoff_factor, double min_scale, double max_scale,
                                                                              double *__restrict__ state, double *__restrict__ ls) {
  double sumsq;
  unsigned long long bad;
  if (!guard_sum_partials(psum, pcnt, nblk, sumsq, bad)) return;
  const double S = ls[0];
  const double norm = sqrt(sumsq) * fabs((double)hyper[3]) / S;      // true units: the arena holds S times the gradient
  double c = 1.0;
  if (clip_global_norm > 0.f) {
    c = (double)clip_global_norm / (norm + 1e-6);
    if (!(c < 1.0)) c = 1.0;
  }
  const double skip = bad > 0 ? 1.0 : 0.0;
  state[0] = norm;
  state[1] = c / S;                    // the update multiplies the gradients with it: clips and unscales in one product
  state[2] = skip;
  state[3] = (double)bad;
  state[4] += 1.0;
  state[5] += skip;
  state[6] = skip != 0.0 ? state[6] + 1.0 : 0.0;
  state[7] = sumsq;
  // the policy
  double scale = S, clean = ls[2];
  if (skip != 0.0) {
    const double want = S * backoff_factor;
    scale = want < min_scale ? min_scale : want;
    if (scale < S) ls[4] += 1.0;
    if (want < min_scale) ls[6] += 1.0;
    clean = 0.0;
  } else {
    clean += 1.0;
    if (growth_interval > 0 && clean == (double)growth_interval) {
      const double want = S * growth_factor;
      scale = want > max_scale ? max_scale : want;
      if (scale > S) ls[3] += 1.0;
      if (want > max_scale) ls[5] += 1.0;
      clean = 0.0;
    }
  }
  ls[0] = scale;
  ls[1] = S;
  ls[2] = clean;
}

struct AuxDesc {
  float *ptr;
  int32_t off, n;
};
static_assert(sizeof(AuxDesc) == 16, "sn_aux_shadow: the record is {float *ptr; int32 off; int32 n}");

// one block per vector; mode 0: shadow <- ptr, mode 1: ptr <- shadow when the guard skipped the step
__global__ __launch_bounds__(256) void aux_shadow_kernel(const AuxDesc *__restrict__ desc, float *__restrict__ shadow, int mode,
                                                         const double *__restrict__ state) {
  const AuxDesc d = desc[blockIdx.x];
  float *__restrict__ sh = shadow + d.off;
  if (mode == 0) {
    for (int i = threadIdx.x; i < d.n; i += 256) sh[i] = d.ptr[i];
    return;
  }
  if (state[2] == 0.0) return;
  for (int i = threadIdx.x; i < d.n; i += 256) d.ptr[i] = sh[i];
}

// a positive power of two that a float holds exactly (the loss kernels read the scale as a float)
bool pow2(double x) {
  int e;
  return x > 0.0 && isfinite(x) && frexp(x, &e) == 0.5;
}
bool pow2_float(double x) { return pow2(x) && x >= 0x1p-126 && x <= 0x1p127; }

}  // namespace

SN_EXPORT int sn_softmax_output_bwd_scaled(const float *p, const float *label, float *grad, long outer, int K, long inner,
                                           float ignore_label, int use_ignore, float grad_scale, int normalize_valid, int *ws,
                                           const double *d_ls, sn_stream_t stream) {
  SN_REQUIRE(p && label && grad && ws && d_ls, "sn_softmax_output_bwd_scaled: null pointer");
  SN_REQUIRE(outer > 0 && K > 0 && inner > 0, "sn_softmax_output_bwd_scaled: bad shape");
  SN_REQUIRE(((uintptr_t)d_ls & 7) == 0, "sn_softmax_output_bwd_scaled: d_ls must be 8-byte aligned");
  hipStream_t s = sn_stream(stream);
  if (normalize_valid) {
    const int rc = sn_softmax_count_valid(label, outer * inner, ignore_label, use_ignore, ws, s);
    if (rc != SN_OK) return rc;
  }
  if (softmax_rows_ok(p, grad, K, inner)) {
    const int R = softmax_rows_per_block(K);
    SN_REQUIRE((outer + R - 1) / R < (1l << 31), "sn_softmax_output_bwd_scaled: too many rows");
    hipLaunchKernelGGL(softmax_rows_bwd_scaled_kernel, dim3((unsigned)((outer + R - 1) / R)), dim3(256), 0, s, p, label, grad, outer, K,
                       R, sn_div_make((unsigned)K), ignore_label, use_ignore, grad_scale, normalize_valid, (const int *)ws, d_ls);
  } else {
    hipLaunchKernelGGL(softmax_bwd_scaled_kernel, dim3(softmax_strided_blocks(outer * inner)), dim3(256), 0, s, p, label, grad, outer,
                       K, inner, ignore_label, use_ignore, grad_scale, normalize_valid, (const int *)ws, d_ls);
  }
  SN_CHECK_LAUNCH();
  return SN_OK;
}

SN_EXPORT int sn_fill_scaled_f32(float *out, long n, float value, const double *d_ls, sn_stream_t stream) {
  SN_REQUIRE(out && d_ls && n > 0, "sn_fill_scaled_f32: bad arguments");
  SN_REQUIRE(((uintptr_t)d_ls & 7) == 0, "sn_fill_scaled_f32: d_ls must be 8-byte aligned");
  hipLaunchKernelGGL(fill_scaled_kernel, dim3(sn_blocks(n, 8192)), dim3(256), 0, sn_stream(stream), out, n, value, d_ls);
  SN_CHECK_LAUNCH();
  return SN_OK;
}

SN_EXPORT int sn_grad_guard_scaled(const float *d_grad, long n, const float *d_hyper, float clip_global_norm, int max_blocks,
                                   int growth_interval, double growth_factor, double backoff_factor, double min_scale,
                                   double max_scale, void *d_ws, double *d_state, double *d_ls, sn_stream_t stream) {
  SN_REQUIRE(d_ls && ((uintptr_t)d_ls & 7) == 0, "sn_grad_guard_scaled: d_ls must be a non-null, 8-byte aligned pointer");
  SN_REQUIRE(pow2(growth_factor) && pow2(backoff_factor) && pow2_float(min_scale) && pow2_float(max_scale),
             "sn_grad_guard_scaled: growth_factor %g, backoff_factor %g, min_scale %g and max_scale %g must be positive powers of two "
             "(the scales within 2^-126 .. 2^127)", growth_factor, backoff_factor, min_scale, max_scale);
  SN_REQUIRE(growth_factor >= 1.0, "sn_grad_guard_scaled: growth_factor %g < 1", growth_factor);
  SN_REQUIRE(backoff_factor <= 1.0, "sn_grad_guard_scaled: backoff_factor %g > 1", backoff_factor);
  SN_REQUIRE(min_scale <= max_scale, "sn_grad_guard_scaled: min_scale %g > max_scale %g", min_scale, max_scale);
  SN_REQUIRE(growth_interval >= 0, "sn_grad_guard_scaled: growth_interval = %d", growth_interval);
  int nblk = 0;
  const int rc = sn_grad_guard_partials("sn_grad_guard_scaled", d_grad, n, d_hyper, clip_global_norm, max_blocks, d_ws, d_state, &nblk,
                                        sn_stream(stream));
  if (rc != SN_OK) return rc;
  double *psum = (double *)d_ws;
  unsigned long long *pcnt = (unsigned long long *)(psum + nblk);
  hipLaunchKernelGGL(grad_guard_scaled_finalize_kernel, dim3(1), dim3(kThreads), 0, sn_stream(stream), (const double *)psum,
                     (const unsigned long long *)pcnt, nblk, d_hyper, clip_global_norm, growth_interval, growth_factor, backoff_factor,
                     min_scale, max_scale, d_state, d_ls);
  SN_CHECK_LAUNCH();
  return SN_OK;
}

SN_EXPORT int sn_aux_shadow(const void *desc, int n_desc, float *d_shadow, int mode, const double *d_state, sn_stream_t stream) {
  SN_REQUIRE(n_desc >= 0 && (mode == 0 || mode == 1), "sn_aux_shadow: n_desc = %d, mode = %d", n_desc, mode);
  if (n_desc == 0) return SN_OK;
  SN_REQUIRE(desc && d_shadow && (mode == 0 || d_state), "sn_aux_shadow: null pointer");
  SN_REQUIRE(((uintptr_t)desc & 7) == 0 && ((uintptr_t)d_shadow & 3) == 0 && ((uintptr_t)d_state & 7) == 0,
             "sn_aux_shadow: desc and d_state must be 8-byte aligned, d_shadow 4-byte aligned");
  hipLaunchKernelGGL(aux_shadow_kernel, dim3(n_desc), dim3(256), 0, sn_stream(stream), (const AuxDesc *)desc, d_shadow, mode, d_state);
  SN_CHECK_LAUNCH();
  return SN_OK;
}
