/*
 * salun.h — C-ABI of the MI355X-native SalUn hot path (libsalun.so, gfx950).
 *
 * This is the drop-in boundary.  The reference
 * (OPTML-Group/Unlearn-Saliency) is 100 % Python and has no FFI of its own; each
 * entry point below replaces a *sequence of stock ATen launches* issued from a
 * Python loop over parameter tensors.  The reference sequence every function
 * replaces is cited as  <file>:<lines>  relative to the reference checkout.
 *
 * Conventions (all functions):
 *   - plain pointers and sizes only; no torch / HIP types in the signatures.
 *     `stream` is a hipStream_t passed as void* (NULL = the null stream).
 *   - every pointer marked "dev" is a device pointer owned by the caller; nothing
 *     is retained after return; all work is stream-ordered, nothing synchronises
 *     the host, nothing allocates.  Scratch memory is passed in by the caller
 *     (`ws`, `ws_bytes`), sized by the matching *_workspace_bytes() query.
 *   - return value: 0 (SALUN_OK) or a negative errno-style code; never throws,
 *     never aborts.  salun_strerror() names a code.
 *   - vectors are the *flat* concatenation of all parameter tensors in
 *     named_parameters() order, each tensor row-major.
 *     Pointers should be 16-byte aligned for the fast path; any alignment is
 *     accepted (a scalar path is used).
 *   - masks are uint8 0/1 (1 byte per weight) inside the library; the reference's
 *     on-disk format (int64 0/1) is produced/consumed by the two converters.
 *   - fp32 arithmetic is IEEE round-to-nearest with the operation order stated
 *     per function (compiled with -ffp-contract=off; fused multiply-adds appear
 *     only where written as fma()).  oracle/salun_oracle.c restates exactly the
 *     same order on the CPU, so GPU-vs-oracle comparisons are bit-exact for the
 *     element-wise kernels and for the mask.
 */
#ifndef SALUN_H
#define SALUN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SALUN_OK 0
#define SALUN_EINVAL (-22)   /* bad argument (null pointer, negative size, nk out of range) */
#define SALUN_ENOSPC (-28)   /* workspace too small */
#define SALUN_EIO (-5)       /* HIP launch / runtime error */

#define SALUN_MAX_THRESHOLDS 16

typedef void *salun_stream_t; /* hipStream_t */

/* Library identification: major*10000 + minor*100 + patch. */
int salun_version(void);
/* Static string for a return code. */
const char *salun_strerror(int code);
/* Target ISA the kernels were compiled for ("gfx950"). */
const char *salun_arch(void);
/* Measurement tooling (tools/clock_probe.py): one wave samples the shader-cycle counter against the 100 MHz constant
 * counter `samples` times, `spins` s_sleep(127) apart: out[2i] = shader cycles, out[2i+1] = 100 MHz ticks.  Launched on a
 * stream of its own beside a workload it reads the clock the chip sustains under that workload. */
int salun_clock_probe(unsigned long long *out /*dev, 2*samples*/, int samples, int spins, salun_stream_t stream);

/* ------------------------------------------------------------------ K1 --
 * Saliency accumulation:   acc[i] <- acc[i] + (g[i] * scale)      (2 roundings)
 * Replaces the per-tensor loop  `gradients[name] += param.grad.data`
 *   Classification/generate_mask.py:41-44, DDPM/runners/diffusion.py:992-996,
 *   SD/train-scripts/generate_mask.py:66-69,171-174.
 * scale = 1 for Classification/SD.  For DDPM the per-batch clip of
 * runners/diffusion.py:985-990 is folded in: if `sqnorm` (dev, 1 float, the
 * squared global L2 norm of g from salun_grad_sqnorm) is non-NULL the scale is
 * computed on the device as  min(1, max_norm / (sqrt(*sqnorm) + 1e-6))  — the
 * clip_grad_norm_ coefficient — and `scale` is ignored.
 * Algorithmic traffic: 12 B / element. */
int salun_saliency_accumulate(float *acc /*dev*/, const float *g /*dev*/,
                              double scale, const float *sqnorm /*dev or NULL*/,
                              double max_norm, int64_t n, salun_stream_t stream);

/* ------------------------------------------------------------------ K2 --
 * Global top-k saliency mask for nk thresholds at once.
 * Replaces  abs_ -> -cat(flatten) -> argsort -> argsort -> (ranks < k)
 *   Classification/generate_mask.py:46-80, DDPM/runners/diffusion.py:998-1037,
 *   SD/train-scripts/generate_mask.py:71-106,176-209.
 * For threshold j:  masks_out[j][i] = 1  iff  rank_desc(|acc[i]|) < ks[j], where
 * rank_desc orders by |acc| descending, ties by flat index ascending (the
 * `argsort(stable=True)` reading of the reference) and NaN
 * after every number.  popcount(masks_out[j]) == min(max(ks[j],0), n) exactly.
 * `acc` is NOT modified (the abs is fused).  ks[] and masks_out[] are HOST
 * arrays (read before return); masks_out[j] are device pointers to n bytes.
 * 1 <= nk <= SALUN_MAX_THRESHOLDS.
 * Algorithmic traffic: 4 B read + nk B written per element.
 * Implementation (csrc/salun_topk.hip): for n >= 8192 and 16-B aligned input the vector is read ONCE — a hashed
 * sample brackets every threshold, one streaming pass writes the masks outside the brackets and compacts the ~4 % of
 * elements inside them, and the exact threshold is resolved among those candidates.  k >= n selects everything without
 * a select; exact zeros (a real accumulator holds several per cent of them) are counted instead of compacted, and a
 * threshold that lands among them is finished by a tie pass in flat-index order; candidates a workgroup's slab cannot
 * take (a layer whose magnitudes sit at the threshold) go to a shared spill row.  A persistent full-scan radix select
 * (3 histogram passes + 1 write pass, grid barriers) handles small / unaligned inputs and is the device-side fallback
 * when a bracket misses, heavy ties at a non-zero key overflow a buffer, or a threshold lies among NaNs — the resulting
 * mask is the same function of the input either way.
 * salun_mask_topk_ex takes flags:
 *   SALUN_TOPK_FORCE_FULL_SCAN  skip the single-read route (tests / A-B timing)
 *   SALUN_TOPK_VALUES_ONLY      no masks are written (masks_out may be NULL); only the thresholds are published
 * salun_mask_topk == salun_mask_topk_ex with flags 0. */
#define SALUN_TOPK_FORCE_FULL_SCAN 1u
#define SALUN_TOPK_VALUES_ONLY 2u
size_t salun_mask_topk_workspace_bytes(int64_t n, int nk);
int salun_mask_topk(const float *acc /*dev*/, int64_t n, const int64_t *ks /*host*/,
                    int nk, uint8_t *const *masks_out /*host array of dev ptrs*/,
                    void *ws /*dev*/, size_t ws_bytes, salun_stream_t stream);
int salun_mask_topk_ex(const float *acc /*dev*/, int64_t n, const int64_t *ks /*host*/,
                       int nk, uint8_t *const *masks_out /*host array of dev ptrs, or NULL*/,
                       void *ws /*dev*/, size_t ws_bytes, unsigned flags, salun_stream_t stream);
/* Synchronises the stream: which route finished the last call on this ws (1 = single-read, 2 = full scan) and
 * whether a grid barrier of the full scan timed out (*error_out = 1: the masks / thresholds of that call are INVALID).
 * The full scan synchronises its workgroups with a bounded software grid barrier; called directly (small or
 * unaligned inputs, SALUN_TOPK_FORCE_FULL_SCAN) it is launched cooperatively, so the runtime guarantees the
 * co-residency the barrier needs; as the fallback behind the single-read route it is a plain launch.  Either way a
 * time-out is never silent: callers that hand masks to a file or an optimizer check this status (one host sync, the
 * Python wrappers' `check=True`), callers that must not synchronise receive NaN from salun_mask_topk_thresholds. */
int salun_mask_topk_status(const void *ws /*dev*/, int *route_out /*host*/, int *error_out /*host*/,
                           salun_stream_t stream);
/* After salun_mask_topk on the same ws: copies the nk selected thresholds
 * (as fp32 |acc| values; NaN if the k-th element is a NaN OR if the select failed — see salun_mask_topk_status;
 * +inf for k <= 0, -1 for k > n) to a device array, 4*nk bytes.  Used by the proximal step (K9) as the
 * device-resident threshold. */
int salun_mask_topk_thresholds(const void *ws /*dev*/, int nk, float *tau_out /*dev*/,
                               salun_stream_t stream);

/* Mask format converters for the file boundary (reference masks are int64 0/1
 * tensors: `torch.zeros_like(tensor_ranks)`, generate_mask.py:76-79).
 * i64 -> u8 maps any non-zero to 1. */
int salun_mask_u8_to_i64(const uint8_t *m /*dev*/, int64_t *out /*dev*/, int64_t n,
                         salun_stream_t stream);
int salun_mask_i64_to_u8(const int64_t *m /*dev*/, uint8_t *out /*dev*/, int64_t n,
                         salun_stream_t stream);
/* Number of ones -> *count (dev, 1 int64). Workspace: salun_reduce_workspace_bytes(n). */
int salun_mask_popcount(const uint8_t *m /*dev*/, int64_t n, int64_t *count /*dev*/,
                        void *ws /*dev*/, size_t ws_bytes, salun_stream_t stream);

/* --------------------------------------------------------------- K3+K4 --
 * Masked SGD-momentum step, one launch for the whole model.
 * Replaces  _apply_mask_to_grads -> torch.optim.SGD.step -> _restore_masked_params
 *   Classification/unlearn/RL.py:11-14, unlearn/impl.py:68-73 (SGD, dampening 0,
 *   nesterov off), RL.py:17-34  (same helpers in GA.py/FT.py/boundary_*.py and
 *   trainer/train.py:58-61,104-107).
 * Where m[i]==1 (or m==NULL: unmasked plain SGD):
 *     d   = fma(wd, p, g)                     (d = g when wd == 0)
 *     buf = first_step ? d : (mu*buf) + d     (mu*buf rounded, then added)
 *     p   = fma(-lr, buf, p)
 * Where m[i]==0:  p is left bit-identical (it equals theta0 by the invariant the
 * reference's restore enforces every step), buf = 0.
 * `mu == 0` means "no momentum": buf is neither read nor written, may be NULL.
 * lr/mu/wd are doubles (Python floats) rounded to fp32 once, as torch does.
 * Algorithmic traffic: 21 B / element (r p,g,buf,m ; w p,buf). */
int salun_masked_sgd_step(float *p /*dev*/, const float *g /*dev*/, float *buf /*dev*/,
                          const uint8_t *m /*dev or NULL*/, double lr, double mu,
                          double wd, int first_step, int64_t n, salun_stream_t stream);

/* ------------------------------------------------------------------ K5 --
 * Squared global L2 norm of the flat gradient: *out = sum_i g[i]^2  (fp32 result,
 * accumulated per thread in fp32 lanes and across threads/blocks in fp64, fixed
 * reduction tree => run-to-run deterministic).
 * Replaces the per-tensor norms of torch.nn.utils.clip_grad_norm_
 *   DDPM/runners/diffusion.py:582-587,985-990.
 * Algorithmic traffic: 4 B / element. */
size_t salun_reduce_workspace_bytes(int64_t n);
int salun_grad_sqnorm(const float *g /*dev*/, int64_t n, float *out /*dev*/,
                      void *ws /*dev*/, size_t ws_bytes, salun_stream_t stream);

/* Masked Adam step (clip -> mask -> Adam), one launch for the whole model.
 * Replaces  clip_grad_norm_ -> `param.grad *= mask[name].to(device)` -> Adam.step
 *   DDPM/runners/diffusion.py:582-593 with DDPM/functions/__init__.py:9-18
 *   (Adam, amsgrad off), SD/train-scripts/random_label.py:129-139,
 *   SD/train-scripts/nsfw_removal.py:150-160.
 *     s   = sqnorm ? min(1, max_norm/(sqrt(*sqnorm)+1e-6)) : gscale
 *     ge  = (g*s) * m                 (m==NULL: ge = g*s)
 *     ge  = fma(wd, p, ge)            (only when wd != 0)
 *     m1  = (b1*m1) + ((1-b1)*ge)
 *     v   = (b2*v)  + ((1-b2)*ge)*ge
 *     den = sqrt(v)/sqrt(1-b2^step) + eps
 *     p   = p + (-(lr/(1-b1^step))) * (m1/den)
 * Hyper-parameters are doubles (Python floats); 1-b1, 1-b2, the bias corrections
 * and lr/(1-b1^step) are evaluated on the host in double and only then rounded to
 * fp32, like the Python scalars torch.optim.Adam hands to its fp32 kernels.
 * step is 1-based.  Algorithmic traffic: 29 B / element. */
int salun_masked_adam_step(float *p /*dev*/, const float *g /*dev*/, float *m1 /*dev*/,
                           float *v /*dev*/, const uint8_t *mask /*dev or NULL*/,
                           const float *sqnorm /*dev or NULL*/, double max_norm,
                           double gscale, double lr, double b1, double b2, double eps,
                           double wd, int step, int64_t n, salun_stream_t stream);

/* The same step with its step-dependent scalars taken from DEVICE memory — for callers that replay
 * identical kernel arguments every step (the host cannot pass t):
 *   salun_adam_coefficients: ++(*step) on the stream, then coef = { sqrt(1 - b2^t), -lr / (1 - b1^t) } in the same
 *     double arithmetic as salun_masked_adam_step;
 *   salun_masked_adam_step_coef: salun_masked_adam_step reading those two floats instead of (lr, step). */
int salun_adam_coefficients(int64_t *step /*dev*/, double lr, double b1, double b2, float *coef /*dev [2]*/,
                            salun_stream_t stream);
int salun_masked_adam_step_coef(float *p /*dev*/, const float *g /*dev*/, float *m1 /*dev*/, float *v /*dev*/,
                                const uint8_t *mask /*dev or NULL*/, const float *sqnorm /*dev or NULL*/,
                                double max_norm, double gscale, const float *coef /*dev [2]*/, double b1, double b2,
                                double eps, double wd, int64_t n, salun_stream_t stream);

/* ----------------------------------------------------------------- K20 --
 * Masked Adam step + EMA of the parameters in ONE pass (training from scratch: DDPM/runners/diffusion.py:238-250,
 * 445-457 with DDPM/models/ema.py:28-36).  Per element: exactly salun_masked_adam_step (same device function, p / m1 / v
 * bit-identical to it), then with the new p still in registers
 *     shadow = shadow + w * (p - shadow),   w = (float)(1 - mu)      (1 - mu evaluated in double on the host)
 * which is Tensor.lerp_(p, 1 - mu) for a weight below 0.5 (ATen/native/Lerp.h): the product and the sum are one fused
 * multiply-add, as in ATen's device code for gfx950 (v_sub_f32, then v_fma_f32).
 * p, g, m1, v, shadow must be five distinct buffers (SALUN_EINVAL otherwise, nothing is launched).
 * The two entry points mirror salun_masked_adam_step / salun_masked_adam_step_coef.
 * Algorithmic traffic: 36 B / element (read p, g, m1, v, shadow; write p, m1, v, shadow); 37 with a mask —
 * against 28 (29) + 12 for the Adam kernel followed by lerp_. */
int salun_adam_ema_step(float *p /*dev*/, const float *g /*dev*/, float *m1 /*dev*/, float *v /*dev*/,
                        float *shadow /*dev*/, const uint8_t *mask /*dev or NULL*/,
                        const float *sqnorm /*dev or NULL*/, double max_norm, double gscale, double lr, double b1,
                        double b2, double eps, double wd, double mu, int step, int64_t n, salun_stream_t stream);
int salun_adam_ema_step_coef(float *p /*dev*/, const float *g /*dev*/, float *m1 /*dev*/, float *v /*dev*/,
                             float *shadow /*dev*/, const uint8_t *mask /*dev or NULL*/,
                             const float *sqnorm /*dev or NULL*/, double max_norm, double gscale,
                             const float *coef /*dev [2]*/, double b1, double b2, double eps, double wd, double mu,
                             int64_t n, salun_stream_t stream);

/* ------------------------------------------------------------------ K6 --
 * Forward diffusion sample:  xt = x0*sqrt_ab[t[b]] + e*sqrt_1mab[t[b]]
 * Replaces  DDPM/functions/losses.py:31-32, runners/diffusion.py:558-559,973-974.
 * x0,e,xt: (B, chw) row-major; sqrt_ab/sqrt_1mab: (T,) tables; t: (B,) int64. */
int salun_qsample(const float *x0 /*dev*/, const float *e /*dev*/,
                  const float *sqrt_ab /*dev*/, const float *sqrt_1mab /*dev*/,
                  const int64_t *t /*dev*/, int64_t T, float *xt /*dev*/, int64_t B,
                  int64_t chw, salun_stream_t stream);

/* Squared-error loss + gradient in one pass over (B, chw) tensors a and b:
 *     per_sample[s] = sum_j (a[s,j]-b[s,j])^2          (optional output)
 *     *loss         = coef * sum_s per_sample[s]
 *     dloss_db[s,j] = -2*coef*(a[s,j]-b[s,j])           (optional output)
 * eps-MSE  `(e-out).square().sum((1,2,3)).mean(0)`  = (a=e, b=out, coef=1/B)
 *   DDPM/functions/losses.py:34-37, runners/diffusion.py:980;
 * nn.MSELoss(pseudo, out) = (a=pseudo, b=out, coef=1/(B*chw))
 *   runners/diffusion.py:507,570, SD random_label.py:113-127.
 * Reduction order is fixed (deterministic).  Workspace: salun_sqerr_workspace_bytes(B, chw). */
size_t salun_sqerr_workspace_bytes(int64_t B, int64_t chw);
int salun_sqerr_loss(const float *a /*dev*/, const float *b /*dev*/, int64_t B,
                     int64_t chw, double coef, float *loss /*dev*/,
                     float *per_sample /*dev or NULL*/, float *dloss_db /*dev or NULL*/,
                     void *ws /*dev*/, size_t ws_bytes, salun_stream_t stream);

/* ------------------------------------------------------------------ K7 --
 * Diagonal empirical Fisher accumulation:  F += (tmp*tmp)/n_data ; tmp = 0.
 * Replaces  DDPM/runners/diffusion.py:176-183
 *   (`fisher += tmp**2 / len(dataset)`, then tmp re-zeroed).   16 B / element. */
int salun_fim_square_accumulate(float *F /*dev*/, float *tmp /*dev*/, double n_data,
                                int64_t n, salun_stream_t stream);

/* ------------------------------------------------------------------ K8 --
 * fp32 2-D convolution on the matrix cores (v_mfma_f32_32x32x2_f32, exact fp32 FMA chains), NCHW
 * activations, OIHW weights read in place from the flat arena.  Replaces the library convolution calls
 * autograd issues for `nn.Conv2d` forward / backward in the models on the path
 *   (Classification/models/ResNet.py:58-74,218-220; DDPM/models/diffusion.py:54-56,71-73,103-122,154-165,
 *    245-247,325-327) — see DESIGN.md §3 for why (the library picks naive kernels for these fp32 shapes).
 * Supported: square filter R in {1,3}, stride in {1,2}, dilation 1, groups 1; `pad` is the low-side
 * (top/left) padding, the high side is implied by P,Q; Q (forward / weight) resp. W (backward-data) must be
 * a power of two <= 128 and the pixel space must tile (see csrc/salun_conv.hip make_geom).  Unsupported
 * shapes return SALUN_EINVAL and the caller uses the library convolution.
 *   forward        y[N,K,P,Q]  = conv(x[N,C,H,W], w[K,C,R,R]) (+ bias[K] if non-NULL)
 *   backward_data  dx[N,C,H,W] = conv_transpose(dy[N,K,P,Q], w)
 *   backward_weight dw[K,C,R,R] (= or += if accumulate) sum over n,p,q of dy * x; deterministic
 *                  (pixel range split over workgroups -> partials in `ws` -> fixed-order reduce). */
int salun_conv2d_forward(const float *x /*dev*/, const float *w /*dev*/, const float *bias /*dev or NULL*/,
                         float *y /*dev*/, int N, int C, int H, int W, int K, int R, int stride, int pad,
                         int P, int Q, salun_stream_t stream);
/* Forward with the epilogue of a diffusion ResnetBlock (DDPM/models/diffusion.py:113-127 of the reference:
 * `h = conv1(..); h = h + temb_proj(..)[:, :, None, None]` and `return x + h`) folded in:
 *   y = conv2d(x, w) + bias[k] + nbias[n][k] + addend[n][k][p][q]      (each term optional, added in that order —
 * the order the reference's separate adds produce).  addend must not alias y.  nbias / addend are carried by dedicated
 * instantiations of the kernel (stride 1, C a multiple of the staging chunk: 8, or 32 for R = 1, 16-byte aligned
 * weights); any other shape with them returns SALUN_EINVAL. */
int salun_conv2d_forward_fused(const float *x /*dev*/, const float *w /*dev*/, const float *bias /*dev or NULL*/,
                               const float *nbias /*dev [N,K] or NULL*/, const float *addend /*dev [N,K,P,Q] or NULL*/,
                               float *y /*dev*/, int N, int C, int H, int W, int K, int R, int stride, int pad,
                               int P, int Q, void *ws /*dev or NULL*/, size_t ws_bytes, salun_stream_t stream);
/* Under-filled launches (an output small enough for <= 256 workgroups, e.g. the 4x4 level of the DDPM U-Net: half the
 * CUs idle) are split over the reduction channels when a workspace is passed: S <= 8 workgroups per output tile write
 * partial images, a second small kernel adds them in fixed order together with the epilogue terms (deterministic; the
 * rounding differs from the unsplit launch's).  salun_conv2d_data_workspace_bytes: bytes for an OUTPUT of
 * [N, outC, outH, outW] (forward: K, P, Q and the forward stride; backward-data: C, H, W and conv_stride 1); 0 when
 * the launch would not be split.  ws == NULL: never split. */
size_t salun_conv2d_data_workspace_bytes(int N, int outC, int outH, int outW, int R, int conv_stride);
int salun_conv2d_backward_data_ws(const float *dy /*dev*/, const float *w /*dev*/, const float *addend /*dev or NULL*/,
                                  float *dx /*dev*/, int N, int C, int H, int W, int K, int R, int stride, int pad,
                                  int P, int Q, void *ws /*dev or NULL*/, size_t ws_bytes, salun_stream_t stream);
int salun_conv2d_backward_data(const float *dy /*dev*/, const float *w /*dev*/, float *dx /*dev*/, int N, int C,
                               int H, int W, int K, int R, int stride, int pad, int P, int Q,
                               salun_stream_t stream);
/* dx = backward_data(dy, w) + addend  (addend: [N,C,H,W] or NULL; addend == dx accumulates in place).  The residual
 * branch's gradient of a ResNet block is folded into the convolution's epilogue instead of a separate add pass. */
int salun_conv2d_backward_data_add(const float *dy /*dev*/, const float *w /*dev*/, const float *addend /*dev or NULL*/,
                                   float *dx /*dev*/, int N, int C, int H, int W, int K, int R, int stride, int pad,
                                   int P, int Q, salun_stream_t stream);
/* Bias gradient of a convolution: out[k] (= or +=, `accumulate`) sum over n, p, q of dy[n][k][p][q] — what the reference
 * gets from autograd's `sum(dim=(0, 2, 3))` + AccumulateGrad for every biased `nn.Conv2d` of the diffusion U-Nets
 * (DDPM/models/diffusion.py:20-75, SD openaimodel.py `conv_nd`).  One streaming pass, 4 B per element of dy;
 * deterministic (fixed-order partial sums).  `out` may be the parameter's slice of the flat gradient arena. */
size_t salun_channel_sum_workspace_bytes(int N, int K);
int salun_channel_sum(const float *dy /*dev*/, float *out /*dev, K floats*/, int N, int K, int HW, int accumulate,
                      void *ws /*dev*/, size_t ws_bytes, salun_stream_t stream);
size_t salun_conv2d_wgrad_workspace_bytes(int N, int C, int K, int R, int P, int Q);
int salun_conv2d_backward_weight(const float *x /*dev*/, const float *dy /*dev*/, float *dw /*dev*/, int N, int C,
                                 int H, int W, int K, int R, int stride, int pad, int P, int Q, int accumulate,
                                 void *ws /*dev*/, size_t ws_bytes, salun_stream_t stream);
/* The same with scheduling hints.  SALUN_WGRAD_SHARED: the launch runs on a side stream BESIDE other kernels of the
 * step (resblock.py overlaps backward-weight with backward-data and the normalisation backward): 3x3 / stride 1 layers
 * then keep the register-staged kernel; without the flag they run on the LDS-DMA ring kernel (csrc/salun_conv_ring.hip:
 * 12 - 18 % faster alone).  Both are deterministic; their results differ by the summation order over the pixels. */
#define SALUN_WGRAD_SHARED 1u
int salun_conv2d_backward_weight_ex(const float *x /*dev*/, const float *dy /*dev*/, float *dw /*dev*/, int N, int C,
                                    int H, int W, int K, int R, int stride, int pad, int P, int Q, int accumulate,
                                    unsigned flags, void *ws /*dev*/, size_t ws_bytes, salun_stream_t stream);
/* Which kernel a call of this family runs: the label of the plan the matching entry point would execute, written to
 * `buf` (NUL-terminated; SALUN_ENOSPC if it does not fit), from the very plan functions the entry points launch from.
 * Touches no device.  Returns SALUN_OK, or what the entry point would return for the shape (SALUN_EINVAL: refused).
 *   direction  SALUN_ROUTE_FORWARD (salun_conv2d_forward_fused), SALUN_ROUTE_BACKWARD_DATA (salun_conv2d_backward_data_ws)
 *              or SALUN_ROUTE_BACKWARD_WEIGHT (salun_conv2d_backward_weight_ex)
 *   flags      what a plan needs beyond the shape: SALUN_ROUTE_EPI (nbias or addend given), SALUN_ROUTE_W_UNALIGNED (w),
 *              SALUN_ROUTE_OUT_UNALIGNED (y / dx, the addend or the workspace), SALUN_ROUTE_IN_UNALIGNED (x or dy of
 *              backward-weight) - off a 16-byte boundary; SALUN_WGRAD_SHARED as for salun_conv2d_backward_weight_ex
 *   ws_bytes   of the workspace the call would pass (0: none)
 *   nsplit     (optional) backward-weight: the partial images the reduce kernel adds; else 0
 * Labels: igemm<R,stride[,dgrad]>/<tile>/<fast|slow>/S<split>[/hw-declined][/epi], dgrad_s2<R,pad<p>>/<tile>,
 * dgrad_tap[<RH,RW>/<tile>[/P3] ...][/empty], wgrad_1x1<s>, wgrad_smallc<R,s>, wgrad_ring<W<w>>, wgrad_v<s,nit>,
 * wgrad<R,s,fullC>; <tile> = 256/PT2, 128/KT<n>, 64/KT<n>WK2. */
#define SALUN_ROUTE_FORWARD 0
#define SALUN_ROUTE_BACKWARD_DATA 1
#define SALUN_ROUTE_BACKWARD_WEIGHT 2
#define SALUN_ROUTE_EPI 2u
#define SALUN_ROUTE_W_UNALIGNED 4u
#define SALUN_ROUTE_OUT_UNALIGNED 8u
#define SALUN_ROUTE_IN_UNALIGNED 16u
int salun_conv2d_route(int direction, int N, int C, int H, int W, int K, int R, int stride, int pad, int P, int Q,
                       unsigned flags, size_t ws_bytes, char *buf, size_t buflen, int *nsplit /*or NULL*/);

/* ------------------------------------------------------------------ K8r --
 * 3x3 / stride 1 / pad 1 fp32 convolution, forward and backward-data, with both operands fed by LDS-DMA into a
 * two-stage LDS ring (csrc/salun_conv_ring.hip; round 6) — the same arithmetic as salun_conv2d_forward /
 * salun_conv2d_backward_data for these shapes (bit-identical results: same exact-fp32 FMA chains in the same order),
 * i.e. the BasicBlock convolutions of Classification/models/ResNet.py:77-125 and the ResnetBlock convolutions of
 * DDPM/models/diffusion.py:85-145.  The weights are read from a packed IMAGE of the OIHW tensor (one per direction),
 * rebuilt by salun_conv3x3_pack_weights whenever the parameters changed (once per optimizer step, all layers in one
 * launch):
 *   dgrad = 0: rows = output channels, reduction over input channels   (forward)
 *   dgrad = 1: rows = input channels, reduction over output channels, taps flipped   (backward-data)
 * salun_conv3x3_pack_bytes: size of an image (0: the reduction channel count is not a multiple of 8 — not packable).
 * salun_conv3x3_packed:  y[N,Kout,H,W] = conv3x3(x[N,Cred,H,W], image) (+ bias[Kout]) (+ nbias[N,Kout])
 *   (+ addend[N,Kout,H,W], may alias y); forward: x = input, Cred = C, Kout = K, image dgrad = 0; backward-data:
 *   x = dy, Cred = K, Kout = C, image dgrad = 1.  W in {4, 8, 16, 32}, the pixel space must tile into whole rows /
 *   whole images (SALUN_EINVAL otherwise: the caller uses salun_conv2d_*).  `cfg`: 0 = tile chosen from the problem;
 *   low byte 1..5 pins a tile, bits 8.. the workgroups per CU of the persistent grid (tuning: tools/convring_bench.py). */
size_t salun_conv3x3_pack_bytes(int K, int C, int dgrad);
#define SALUN_PACK_MAX_JOBS 32
typedef struct {
  const float *w;   /* dev, OIHW [K, C, 3, 3] */
  float *img_fwd;   /* dev, salun_conv3x3_pack_bytes(K, C, 0) bytes, or NULL (needs C % 8 == 0) */
  float *img_dgrad; /* dev, salun_conv3x3_pack_bytes(K, C, 1) bytes, or NULL (needs K % 8 == 0) */
  int32_t K, C;
} salun_pack_job_t;
/* Both images of `njobs` layers; one launch per SALUN_PACK_MAX_JOBS layers (`jobs` is a HOST array). */
int salun_conv3x3_pack_weights(const salun_pack_job_t *jobs /*host*/, int njobs, salun_stream_t stream);
int salun_conv3x3_packed(const float *x /*dev*/, const float *img /*dev*/, const float *bias /*dev or NULL*/,
                         const float *nbias /*dev or NULL*/, const float *addend /*dev or NULL*/, float *y /*dev*/,
                         int N, int Cred, int H, int W, int Kout, int cfg, salun_stream_t stream);

/* ------------------------------------------------------------------ K11 --
 * bf16 2-D convolution on the matrix cores (v_mfma_f32_32x32x16_bf16, fp32 accumulators): the convolutions of the
 * Stable-Diffusion U-Net in its bf16 configuration (BASELINE.json configs[4]) — replaces the library calls autograd
 * issues under autocast for the `conv_nd(2, ...)` modules of
 *   SD/ldm/modules/diffusionmodules/openaimodel.py:98-103 (Upsample), :131-133 (Downsample), :192-231 (ResBlock),
 *   :466-470,:716-720 (input / output heads) and SD/ldm/modules/attention.py:230-247 (proj_in / proj_out).
 * Activations are NHWC bf16 (`uint16_t` = raw bf16 bits): x[N][H][W][C], y[N][OH][OW][K]; the master weights stay
 * fp32 OIHW in the flat arena and `salun_conv2d_bf16_pack_weights` writes the bf16 image wp[K][R*R][C] both
 * data kernels read (backward-data reads it transposed, no second image).  Square filter R in {1,3}, stride in
 * {1,2}, symmetric padding <= R-1, C % 32 == 0, K % 32 == 0, 16-B aligned pointers;
 * anything else returns SALUN_EINVAL (`salun_conv2d_bf16_supported` answers without launching), and so does every
 * direction for an empty batch or extent (N, H, W, OH or OW < 1).
 *   forward         y = conv(x, w) + bias[k] + nbias[n][k] + addend[n][oh][ow][k]   (each optional, fp32 / fp32 / bf16)
 *   backward_data   dx = conv_transpose(dy, w) + addend[n][h][w][c]
 *   backward_weight dw[K][C][R][R] fp32 (= or +=): sum over pixels of dy * x, pixel range split over workgroups ->
 *                   fp32 partials in `ws` -> fixed-order reduce (deterministic); db[K] fp32 (optional) = sum of dy. */
int salun_conv2d_bf16_supported(int C, int K, int R, int stride, int pad);
int salun_conv2d_bf16_pack_weights(const float *w /*dev, OIHW*/, uint16_t *wp /*dev*/, int K, int C, int R,
                                   salun_stream_t stream);
/* Every stale weight image of a model in one launch per SALUN_BF16_PACK_MAX_JOBS layers (after an optimizer step all of
 * them are stale; the reference has no counterpart — autocast re-casts each weight on every use,
 * SD/train-scripts/nsfw_removal.py:96-150 under torch.autocast).  `transposed` (R == 1 only): the [C][K] image the Linear
 * layers' input-gradient GEMM reads (what salun_pack_bf16(..., transposed = 1) writes); otherwise wp[K][R*R][C] as above.
 * `jobs` is host memory, read during the call. */
#define SALUN_BF16_PACK_MAX_JOBS 64
typedef struct {
  const float *w;  /* dev, fp32 OIHW [K][C][R][R] */
  uint16_t *wp;    /* dev, bf16 image */
  int32_t K, C, R, transposed;
} salun_bf16_pack_job_t;
int salun_bf16_pack_weights_batch(const salun_bf16_pack_job_t *jobs, int n, salun_stream_t stream);
/* `ws` of forward / backward_data (salun_conv2d_bf16_data_workspace_bytes, may be 0): problems with few output tiles
 * split their reduction over workgroups through fp32 partial tiles there; NULL / too small only disables the split. */
size_t salun_conv2d_bf16_data_workspace_bytes(int N, int H, int W, int C, int K, int R, int stride, int pad);
int salun_conv2d_bf16_forward(const uint16_t *x /*dev*/, const uint16_t *wp /*dev*/, const float *bias /*dev or NULL*/,
                              const float *nbias /*dev or NULL*/, const uint16_t *addend /*dev or NULL*/,
                              uint16_t *y /*dev*/, int N, int H, int W, int C, int K, int R, int stride, int pad,
                              void *ws /*dev or NULL*/, size_t ws_bytes, salun_stream_t stream);
int salun_conv2d_bf16_backward_data(const uint16_t *dy /*dev*/, const uint16_t *wp /*dev*/,
                                    const uint16_t *addend /*dev or NULL*/, uint16_t *dx /*dev*/, int N, int H, int W,
                                    int C, int K, int R, int stride, int pad, void *ws /*dev or NULL*/, size_t ws_bytes,
                                    salun_stream_t stream);
size_t salun_conv2d_bf16_wgrad_workspace_bytes(int N, int H, int W, int C, int K, int R, int stride, int pad);
int salun_conv2d_bf16_backward_weight(const uint16_t *x /*dev*/, const uint16_t *dy /*dev*/, float *dw /*dev*/,
                                      float *db /*dev or NULL*/, int N, int H, int W, int C, int K, int R, int stride,
                                      int pad, int accumulate, void *ws /*dev*/, size_t ws_bytes,
                                      salun_stream_t stream);
/* The same with `dnb` (dev fp32 [N][K] or NULL, N <= 128, always overwritten): the per-image channel sums of dy — the
 * gradient of the forward's `nbias[n][k]` term (a ResBlock's time-embedding projection,
 * SD/ldm/modules/diffusionmodules/openaimodel.py:249-263: `h = h + emb_out[..., None, None]`), from the partial sums the
 * bias gradient is folded from anyway (no fp32 copy of dy, no separate reduction).  db may be NULL then. */
/* The column sums of dy[M][K] (bf16) alone: db[K] (fp32, = or +=; or NULL) and / or dnb[images][K] (fp32, overwritten; or
 * NULL; M = images * pixels, images <= 128) — what the two calls above fold next to dw; for callers that want the
 * per-image sums on another stream than the weight gradient (conv_bf16.py: backward-weight on the side stream, the
 * time-embedding gradient on the compute stream). */
size_t salun_colsum_bf16_workspace_bytes(int K);
int salun_colsum_bf16(const uint16_t *dy /*dev*/, float *db /*dev or NULL*/, float *dnb /*dev or NULL*/, int64_t M, int K,
                      int images, int accumulate, void *ws /*dev*/, size_t ws_bytes, salun_stream_t stream);
int salun_conv2d_bf16_backward_weight_ex(const uint16_t *x /*dev*/, const uint16_t *dy /*dev*/, float *dw /*dev*/,
                                         float *db /*dev or NULL*/, float *dnb /*dev or NULL*/, int N, int H, int W, int C,
                                         int K, int R, int stride, int pad, int accumulate, void *ws /*dev*/,
                                         size_t ws_bytes, salun_stream_t stream);
/* Which kernel, tile and split a call of this family runs (as salun_conv2d_route for the fp32 family): the label of the
 * plan salun_conv2d_bf16_forward / _backward_data / _backward_weight_ex would execute, from the plan functions they launch
 * from (csrc/salun_bf16_plan.h).  Touches no device.  Returns SALUN_OK, or what the entry point would return for the shape
 * (SALUN_EINVAL: refused; backward-weight with `ws_bytes` short of salun_conv2d_bf16_wgrad_workspace_bytes: SALUN_ENOSPC).
 *   direction  SALUN_ROUTE_FORWARD, SALUN_ROUTE_BACKWARD_DATA or SALUN_ROUTE_BACKWARD_WEIGHT
 *   flags      SALUN_ROUTE_OUT_UNALIGNED: forward - y, bias, nbias or addend, backward-weight - dw off a 16-byte boundary;
 *              SALUN_ROUTE_EPI is accepted and changes no plan (both forward kernels carry every epilogue term);
 *              SALUN_ROUTE_RING(v) / SALUN_ROUTE_WGRAD_TN(v): plan as a process started with SALUN_CONV_RING=v (0..3) /
 *              SALUN_WGRAD_TN=v (0, 1) would - without them the query reads the process's switches, as the launch does
 *   ws_bytes   of the workspace the call would pass (0: none - the data kernels then do not split)
 *   nsplit     (optional) the reduction splits of the plan (1: none)
 * Labels: ring<WGM,WGN,NST>, igemm<WM,WN,BK[,dgrad]>/S<split>, wgrad_tn<v<variant>>/S<split>, wgrad_tap<R,stride>/S<split>. */
#define SALUN_ROUTE_RING_SHIFT 8
#define SALUN_ROUTE_RING(v) ((unsigned)((v) + 1) << SALUN_ROUTE_RING_SHIFT)
#define SALUN_ROUTE_WGRAD_TN_SHIFT 12
#define SALUN_ROUTE_WGRAD_TN(v) ((unsigned)((v) + 1) << SALUN_ROUTE_WGRAD_TN_SHIFT)
int salun_conv2d_bf16_route(int direction, int N, int H, int W, int C, int K, int R, int stride, int pad, unsigned flags,
                            size_t ws_bytes, char *buf, size_t buflen, int *nsplit /*or NULL*/);

/* ------------------------------------------------------------------ K12 --
 * GroupNorm (+ SiLU) on bf16 NHWC activations with fp32 statistics — the `GroupNorm32` layers of the SD U-Net in its
 * bf16 configuration (SD/ldm/modules/diffusionmodules/util.py:215-217: `super().forward(x.float()).type(x.dtype)`,
 * followed by nn.SiLU in openaimodel.py:192-196,214-221,716-718; attention.py:228 without SiLU).
 *   forward : y = [silu]( gamma*(x-mean)*rstd + beta ), x / y [N][HW][C] bf16, C % 8 == 0, C % G == 0;
 *             mr[N][G][2] = (mean, rstd) and ab[N][C][2] = (gamma*rstd, beta - mean*gamma*rstd) are outputs the
 *             backward consumes (biased variance, as torch.nn.GroupNorm).
 *   backward: dz = dy * silu'(z); dbeta = sum dz; dgamma = sum dz*xhat; dx = rstd*(dz*gamma - (s1 + xhat*s2)/m)
 *             with s1 = sum_group dz*gamma, s2 = sum_group dz*gamma*xhat.  dgamma / dbeta fp32 (= or += if accumulate).
 * Reductions: per-channel fp32 partials over pixel chunks, folded in fp64 in a fixed order (deterministic). */
size_t salun_gn_bf16_workspace_bytes(int N, int C, int HW, int G);
int salun_gn_bf16_forward(const uint16_t *x /*dev*/, const float *gamma /*dev*/, const float *beta /*dev*/,
                          uint16_t *y /*dev*/, float *mr /*dev*/, float *ab /*dev*/, int N, int C, int HW, int G,
                          double eps, int silu, void *ws /*dev*/, size_t ws_bytes, salun_stream_t stream);
int salun_gn_bf16_backward(const uint16_t *dy /*dev*/, const uint16_t *x /*dev*/, const float *gamma /*dev*/,
                           const float *mr /*dev*/, const float *ab /*dev*/, uint16_t *dx /*dev*/, float *dgamma /*dev*/,
                           float *dbeta /*dev*/, int N, int C, int HW, int G, int silu, int accumulate, void *ws /*dev*/,
                           size_t ws_bytes, salun_stream_t stream);

/* ------------------------------------------------------------------ K13 --
 * Fused scaled-dot-product attention on bf16 tokens (fp32 softmax / accumulation) — replaces
 * `CrossAttention.forward` of SD/ldm/modules/attention.py:168-192 (q.k^T * scale -> softmax -> @ v, which materialises
 * the (B*heads) x Nq x Nk score tensor) for the SD U-Net's self-attention (4096 / 1024 / 256 / 64 tokens) and
 * cross-attention (77 text tokens), 8 heads of D = 40 / 80 / 160 channels (D in {8,16,32,40,64,80,160} supported).
 * Tensors are [B, tokens, H, D] VIEWS: element (b, t, h, d) at b*bs + t*ld + h*D + d (elements); every (token, head)
 * row must be 16-byte aligned.  `lse` ([B*H][Nq] fp32, log2-domain logsumexp of the scaled scores) is the forward's
 * second output and the backward's input; `dsum` is [B*H][Nq] fp32 scratch; dq / dk / dv are written contiguous.
 * `scale` must be positive and finite (SALUN_EINVAL otherwise): the kernels take the running maximum on the raw
 * scores and apply scale*log2(e) afterwards; every attention of the three models uses 1/sqrt(D). */
int salun_attn_supported(int D);
int salun_attn_forward(const uint16_t *q /*dev*/, const uint16_t *k /*dev*/, const uint16_t *v /*dev*/, uint16_t *o /*dev*/,
                       float *lse /*dev or NULL*/, int B, int H, int Nq, int Nk, int D, long long q_bs, int q_ld,
                       long long k_bs, int k_ld, long long v_bs, int v_ld, long long o_bs, int o_ld, double scale,
                       salun_stream_t stream);
int salun_attn_backward(const uint16_t *q /*dev*/, const uint16_t *k /*dev*/, const uint16_t *v /*dev*/,
                        const uint16_t *o /*dev*/, const uint16_t *d_o /*dev*/, const float *lse /*dev*/,
                        uint16_t *dq /*dev*/, uint16_t *dk /*dev*/, uint16_t *dv /*dev*/, float *dsum /*dev*/, int B, int H,
                        int Nq, int Nk, int D, long long q_bs, int q_ld, long long k_bs, int k_ld, long long v_bs, int v_ld,
                        long long o_bs, int o_ld, long long do_bs, int do_ld, double scale, salun_stream_t stream);

/* ------------------------------------------------------------------ K14 --
 * Token-wise layers of the SD transformer blocks on bf16 tokens, fp32 arithmetic, one pass each:
 *   LayerNorm  (SD/ldm/modules/attention.py:196-216, `nn.LayerNorm(dim)` x3 per BasicTransformerBlock):
 *     forward  y[rows][C] = gamma*(x-mean)*rstd + beta, stats[rows][2] = (mean, rstd) for the backward
 *     backward dx, dgamma / dbeta (fp32, = or +=; per-workgroup partials in `ws`, folded in a fixed order)
 *   GEGLU      (attention.py:37-46: `x, gate = proj(x).chunk(2, dim=-1); x * F.gelu(gate)`, erf form):
 *     forward  out[rows][F] = h[:, :F] * gelu(h[:, F:]);  backward dh[rows][2F] from h and d(out).
 * C % 8 == 0, C <= 2048, F % 8 == 0; x / y / h / out 16-byte aligned; gamma / beta may be any fp32 slice. */
size_t salun_ln_bf16_workspace_bytes(int64_t rows, int C);
int salun_ln_bf16_forward(const uint16_t *x /*dev*/, const float *gamma /*dev*/, const float *beta /*dev*/,
                          uint16_t *y /*dev*/, float *stats /*dev or NULL*/, int64_t rows, int C, double eps,
                          salun_stream_t stream);
int salun_ln_bf16_backward(const uint16_t *dy /*dev*/, const uint16_t *x /*dev*/, const float *gamma /*dev*/,
                           const float *stats /*dev*/, uint16_t *dx /*dev*/, float *dgamma /*dev*/, float *dbeta /*dev*/,
                           int64_t rows, int C, int accumulate, void *ws /*dev*/, size_t ws_bytes, salun_stream_t stream);
int salun_geglu_bf16_forward(const uint16_t *h /*dev*/, uint16_t *out /*dev*/, int64_t rows, int F, salun_stream_t stream);
int salun_geglu_bf16_backward(const uint16_t *h /*dev*/, const uint16_t *dy /*dev*/, uint16_t *dh /*dev*/, int64_t rows,
                              int F, salun_stream_t stream);

/* Fused BatchNorm2d (+ residual add) (+ ReLU), NCHW fp32, forward and backward — replaces the
 * bn -> relu / bn -> (+identity) -> relu chains of the classifier blocks
 *   (Classification/models/ResNet.py:108-125,307-309) that run as separate library launches.
 * Semantics of torch.nn.BatchNorm2d: training -> batch statistics (biased variance), running stats updated with
 * `momentum` (unbiased variance); eval -> running statistics.  HW must be a multiple of 4, pointers 16-B aligned.
 *   forward : y = [relu]( gamma*(x-mean)*invstd + beta [+ res] ); save_mean / save_invstd (C floats) are outputs
 *   backward: dz = dy*[y>0] (relu) ; dbeta = sum dz ; dgamma = sum dz*xhat ;
 *             dx = gamma*invstd*(dz - (dbeta + xhat*dgamma)/(N*HW))   (training)   |   gamma*invstd*dz   (eval)
 *             dres = dz  (if non-NULL: gradient of the residual input)
 * Reductions are per-(channel, batch-slice) fp64 partials folded in a fixed order: deterministic.
 * Workspace: salun_bn_workspace_bytes(C). */
size_t salun_bn_workspace_bytes(int C);
int salun_bn_forward(const float *x /*dev*/, const float *res /*dev or NULL*/, float *y /*dev*/,
                     const float *gamma /*dev*/, const float *beta /*dev*/, float *running_mean /*dev or NULL*/,
                     float *running_var /*dev or NULL*/, long long *num_batches_tracked /*dev or NULL: += 1 if training*/,
                     float *save_mean /*dev*/, float *save_invstd /*dev*/,
                     int N, int C, int HW, int training, double momentum, double eps, int relu, void *ws /*dev*/,
                     size_t ws_bytes, salun_stream_t stream);
int salun_bn_backward(const float *dy /*dev*/, const float *y /*dev, needed if relu*/, const float *x /*dev*/,
                      const float *gamma /*dev*/, const float *save_mean /*dev*/, const float *save_invstd /*dev*/,
                      float *dx /*dev*/, float *dres /*dev or NULL*/, float *dgamma /*dev*/, float *dbeta /*dev*/,
                      float *grad_gamma_acc /*dev or NULL: += dgamma*/, float *grad_beta_acc /*dev or NULL: += dbeta*/,
                      int N, int C, int HW, int training, int relu, void *ws /*dev*/, size_t ws_bytes,
                      salun_stream_t stream);

/* Fused GroupNorm (+ SiLU), NCHW fp32, forward and backward — replaces the `nonlinearity(self.norm1(h))` chains of the
 * diffusion U-Nets (DDPM/models/diffusion.py:36-41,118-128,340-352; SD ldm/modules/diffusionmodules/openaimodel.py
 * ResBlock in_layers / out_layers) that run as ~6 library launches forward and ~9 backward per site.
 *   forward : z = [silu]( gamma_c * (x - mean_{n,g}) * rstd_{n,g} + beta_c ),  rstd = 1/sqrt(var_biased + eps);
 *             save_mean / save_rstd (N*G floats) are outputs
 *   backward: dy = dz * silu'(y) with y recomputed from x;  dgamma_c = sum_{n,hw} dy*xhat,  dbeta_c = sum dy;
 *             dx = rstd * (dy*gamma - mean_g(dy*gamma) - xhat * mean_g(dy*gamma*xhat))
 * One workgroup per (image, group); HW must be a power of two >= 4, C % G == 0, pointers 16-B aligned.
 * Reductions are in fixed order (deterministic).  Workspace (backward): salun_gn_workspace_bytes(N, C). */
size_t salun_gn_workspace_bytes(int N, int C);
int salun_gn_forward(const float *x /*dev*/, float *y /*dev*/, const float *gamma /*dev*/, const float *beta /*dev*/,
                     float *save_mean /*dev*/, float *save_rstd /*dev*/, int N, int C, int HW, int G, double eps,
                     int silu, salun_stream_t stream);
int salun_gn_backward(const float *dz /*dev*/, const float *x /*dev*/, const float *gamma /*dev*/,
                      const float *beta /*dev*/, const float *save_mean /*dev*/, const float *save_rstd /*dev*/,
                      float *dx /*dev*/, float *dgamma /*dev*/, float *dbeta /*dev*/,
                      float *grad_gamma_acc /*dev or NULL: += dgamma*/, float *grad_beta_acc /*dev or NULL*/,
                      int N, int C, int HW, int G, int silu, void *ws /*dev*/, size_t ws_bytes,
                      salun_stream_t stream);

/* Backward with the neighbours of a diffusion ResnetBlock folded in: dx (+= addend: the skip branch's gradient,
 * [N,C,HW] or NULL, must not alias dx); nk_sum (N*C floats or NULL) = sum over hw of the dx written, per (image,
 * channel) — the gradient of the per-image channel bias added by the convolution that produced x (the embedding
 * projection); csum / csum_acc (C floats or NULL; need nk_sum) = / += sum over n of nk_sum — that convolution's
 * bias gradient.  All reductions in fixed order. */
int salun_gn_backward_fused(const float *dz /*dev*/, const float *x /*dev*/, const float *gamma /*dev*/,
                            const float *beta /*dev*/, const float *save_mean /*dev*/, const float *save_rstd /*dev*/,
                            const float *addend /*dev or NULL*/, float *dx /*dev*/, float *dgamma /*dev*/,
                            float *dbeta /*dev*/, float *grad_gamma_acc /*dev or NULL*/,
                            float *grad_beta_acc /*dev or NULL*/, float *nk_sum /*dev or NULL*/,
                            float *csum /*dev or NULL*/, float *csum_acc /*dev or NULL*/, int N, int C, int HW, int G,
                            int silu, void *ws /*dev*/, size_t ws_bytes, salun_stream_t stream);

/* ------------------------------------------------------------------ K9 --
 * Proximal (soft-threshold) step of RL_proximal — Classification/unlearn/RL_pro.py:52-60:
 *     d = params - init_params ; threshold = -topk(-|d|, ratio)[0][-1] ;
 *     params = where(d > thr, params - thr, where(d < -thr, params + thr, init_params))
 * as three launches on the flat vectors:  salun_param_diff (out = p - p0, 12 B/elem)  ->  salun_mask_topk on `out`
 * with k = n - ratio + 1 (its k-th largest |d| IS the ratio-th smallest; threshold fetched on the device with
 * salun_mask_topk_thresholds)  ->  salun_soft_threshold_step (12 B/elem), which reads the threshold from device
 * memory — no host round trip.  fp32 arithmetic identical to the reference's tensor expressions.
 * A NaN threshold (a failed select) is propagated: every element of `p` becomes NaN, so the next loss is NaN — never
 * the silent "all weights reset to p0" the three-way comparison would otherwise produce. */
int salun_param_diff(const float *p /*dev*/, const float *p0 /*dev*/, float *out /*dev*/, int64_t n,
                     salun_stream_t stream);
int salun_soft_threshold_step(float *p /*dev*/, const float *p0 /*dev*/, const float *tau /*dev, 1 float*/,
                              int64_t n, salun_stream_t stream);

/* ----------------------------------------------------------------- K10 --
 * EWC (Selective-Amnesia) penalty of DDPM train_forget — DDPM/runners/diffusion.py:343-350:
 *     loss += lambda * sum_name sum( fisher[name] * (param - params_mle[name])**2 )
 * One launch over the flat vectors instead of 334 x 4 per-tensor ops + autograd:
 *     g += (lambda*F) * (2*(p - p_star))      (the term's autograd gradient, fp32)
 *     loss_out[0] = lambda * S, loss_out[1] = S = sum F (p - p_star)^2   (fp64 partials, fixed order)
 * Algorithmic traffic: 20 B / element (r p, p_star, F, g; w g).  Workspace: salun_ewc_workspace_bytes(n). */
size_t salun_ewc_workspace_bytes(int64_t n);
int salun_ewc_penalty_grad(const float *p /*dev*/, const float *p_star /*dev*/, const float *F /*dev*/,
                           float *g /*dev*/, double lambda, float *loss_out /*dev, 2 floats*/, int64_t n,
                           void *ws /*dev*/, size_t ws_bytes, salun_stream_t stream);

/* ------------------------------------------------------------------ K0 --
 * Device-resident CIFAR batch assembly (replaces the host DataLoader path
 * Classification/dataset.py:542-556 + main_random.py:38-48: PIL RandomCrop(32,4)
 * + RandomHorizontalFlip + ToTensor + H2D).
 * data: (num, H, W, C) uint8 resident in HBM; idx: (B,) int64 sample indices;
 * crop: (B,2) int32 (dy,dx) offsets in [0, 2*pad] or NULL (= centred, no crop);
 * flip: (B,) uint8 or NULL; out: (B, C, H, W) fp32 = pixel/255 (ToTensor),
 * zero padding outside the image. */
int salun_image_batch(const uint8_t *data /*dev*/, const int64_t *idx /*dev*/,
                      const int32_t *crop /*dev or NULL*/, const uint8_t *flip /*dev or NULL*/,
                      float *out /*dev*/, int64_t B, int H, int W, int C, int pad,
                      salun_stream_t stream);

/* ----------------------------------------------------------------- K15 --
 * fp32 GEMMs on the matrix cores (v_mfma_f32_32x32x2_f32: exact fp32 FMA chains; results differ from any other fp32
 * GEMM only by summation order) — the Linear layers and the fp32 attention of the diffusion U-Nets, which the
 * reference runs as library GEMMs behind nn.Linear / torch.bmm / einsum:
 *   DDPM/models/diffusion.py:85-145 (temb / cemb dense layers, temb_cemb_proj of every ResnetBlock), :148-192 (AttnBlock);
 *   SD/ldm/modules/attention.py:37-75,149-200, SD/ldm/modules/diffusionmodules/openaimodel.py:428-520 (fp32 configuration).
 *
 * One call computes a TABLE of problems
 *      C_j[M_j, N_j]  (+)=  alpha * sum_{s in segments(j)} A_s . B_s^T   + bias_j[column]
 * with  A_s(i, k) = A[i * a_i + k * a_k],  B_s(j, k) = B[j * b_j + k * b_k]  (element strides, any sign of "transposed"):
 *   x.W^T (forward), dY.W (input gradient), dY^T.x (weight gradient, `accumulate` adds into the flat gradient) and the
 *   channel-major attention operands of the DDPM are the same kernel without a transposing copy.  Several jobs in one
 *   call share the launch (the DDPM's 22 per-block embedding projections); several segments of one job chain their
 *   reductions (the input gradient of those projections: sum_g dproj_g . W_g).
 * Batch: batch_outer x batch_inner instances, instance (o, i) offsets every A / B / C pointer by
 *   o * strides[0|2|4] + i * strides[1|3|5] elements (a_bo a_bi b_bo b_bi c_bo c_bi); batch_strides may be NULL when
 *   there is one instance.
 * Under-filled launches split the reduction into fp32 partial images in `ws` (salun_gemm_f32_workspace_bytes; with a
 * smaller / NULL workspace the call still works, unsplit) folded in a fixed order: no float atomics, deterministic.
 * Limits: njobs <= SALUN_GEMM_MAX_JOBS, nsegs <= SALUN_GEMM_MAX_SEGS, batch <= 65535. */
#define SALUN_GEMM_MAX_JOBS 32
#define SALUN_GEMM_MAX_SEGS 32
typedef struct {
  const float *A /*dev*/, *B /*dev*/;
  int32_t K;                  /* reduction length of this segment */
  int32_t a_i, a_k, b_j, b_k; /* element strides */
} salun_gemm_seg_t;
typedef struct {
  float *C /*dev*/;
  const float *bias /*dev or NULL: one value per column*/;
  int32_t M, N, ldc;
  int32_t seg0, nseg;  /* this job's segments: segs[seg0 .. seg0 + nseg) */
  int32_t accumulate;  /* 0: C = result, 1: C += result */
} salun_gemm_job_t;
size_t salun_gemm_f32_workspace_bytes(const salun_gemm_job_t *jobs /*host*/, int njobs,
                                      const salun_gemm_seg_t *segs /*host*/, int nsegs,
                                      int batch_outer, int batch_inner);
int salun_gemm_f32(const salun_gemm_job_t *jobs /*host*/, int njobs, const salun_gemm_seg_t *segs /*host*/, int nsegs,
                   int batch_outer, int batch_inner, const int64_t *batch_strides /*host[6] or NULL*/,
                   double alpha, void *ws /*dev or NULL*/, size_t ws_bytes, salun_stream_t stream);
/* The route one salun_gemm_f32 call takes, from the very plan the call launches from (no HIP call; pointers are read
 * for null-ness and alignment only).  ws, ws_bytes: the workspace the call would pass (never dereferenced here; a NULL
 * or not 4-byte aligned `ws` is no workspace, for the call and for the query alike).  Returns SALUN_OK, or what the call
 * would return (SALUN_EINVAL: refused).
 *   tile           64 or 128 (square block tile);  tiles: block tiles of all jobs (gridDim.x)
 *   nsplit         split shares launched (1: every workgroup writes C itself); nsplit_wanted: what the shape alone
 *                  asks for (salun_gemm_f32_workspace_bytes sizes that), declined when the workspace is too short
 *   per segment    amode / bmode (0 scalar loads, 1 16-byte loads along k, 2 16-byte loads along the row index) and
 *                  chunk0, the index of its first 16-deep chunk in its job's chunk list
 *   per job        nchunks, per (chunks per split share), empty_shares (shares that start past the last chunk and
 *                  write zeros), tile0 (first block tile), fast_tiles (tiles on the unguarded float4 loop) */
typedef struct {
  int32_t tile, nsplit, nsplit_wanted, njobs, nsegs;
  int64_t tiles;
  int32_t nchunks[SALUN_GEMM_MAX_JOBS], per[SALUN_GEMM_MAX_JOBS], empty_shares[SALUN_GEMM_MAX_JOBS];
  int32_t tile0[SALUN_GEMM_MAX_JOBS], fast_tiles[SALUN_GEMM_MAX_JOBS];
  int32_t amode[SALUN_GEMM_MAX_SEGS], bmode[SALUN_GEMM_MAX_SEGS], chunk0[SALUN_GEMM_MAX_SEGS];
} salun_gemm_route_t;
int salun_gemm_f32_route(const salun_gemm_job_t *jobs /*host*/, int njobs, const salun_gemm_seg_t *segs /*host*/, int nsegs,
                         int batch_outer, int batch_inner, const int64_t *batch_strides /*host[6] or NULL*/,
                         const void *ws /*dev or NULL*/, size_t ws_bytes, salun_gemm_route_t *out /*host*/);
/* out[j] (+)= sum_i x[i * ld + j]: the bias gradient of a Linear layer (the reference: autograd's sum over the token
 * dimension behind nn.Linear).  Two deterministic stages (row slabs, then the slabs in index order). */
size_t salun_colsum_f32_workspace_bytes(int64_t M, int N);
int salun_colsum_f32(const float *x /*dev*/, float *out /*dev*/, int64_t M, int N, int64_t ld, int accumulate,
                     void *ws /*dev*/, size_t ws_bytes, salun_stream_t stream);
/* Row softmax in place: s[r][0..n) <- softmax(s[r][0..n)), rows of leading dimension ld (the P between the two GEMMs of
 * an fp32 attention: DDPM/models/diffusion.py:176, SD attention.py:185).  One wave per row. */
int salun_softmax_rows(float *s /*dev*/, int64_t rows, int n, int ld, salun_stream_t stream);
/* Its backward, written over dp:  dS = scale * P * (dP - sum_j dP_j P_j)  (scale: the attention's 1/sqrt(d), so the two
 * gradient GEMMs that follow need no extra pass). */
int salun_softmax_rows_backward(const float *p /*dev*/, float *dp /*dev*/, int64_t rows, int n, int ld,
                                double scale, salun_stream_t stream);

/* ----------------------------------------------------------------- K16 --
 * bf16 GEMM  y[M, N] = x[M, K] . w[N, K]^T (+ bias[N] fp32) (+ addend[M, N] bf16)  on v_mfma_f32_32x32x16_bf16, fp32
 * accumulation, one rounding to bf16 — the Linear layers of the SD transformer blocks in the bf16 configuration
 * (reference: autocast over SD/ldm/modules/attention.py:37-75 GEGLU / FeedForward, :149-200 to_q / to_k / to_v / to_out).
 * x, w, addend, y: bf16 row-major; both operand tiles go global -> LDS directly (global_load_lds_dwordx4, bank swizzle on
 * the source address).  The input gradient dX = dY . W is the same call on the transposed image (salun_pack_bf16 with
 * transposed = 1).  Requirements: K % 64 == 0, N % 64 == 0, 16-byte aligned pointers (salun_gemm_bf16_supported);
 * SALUN_EINVAL otherwise.  variant: 0 = choose the tile; 1..13 pin one (A/B measurements): 1 / 2 = 128 tokens x 128
 * features double- / single-buffered, 3 / 4 = 256 x 64 likewise, 5 / 6 = the persistent forms of 1 / 3, 7..13 = the LDS ring
 * (128 x 128 x 4 stages, 256 x 128 x 3, 256 x 64 x 3, 128 x 128 x 3, and 11..13 = 8 / 7 / 9 with 32-deep stages).  The
 * 128-feature tiles (1, 2, 5, 7, 8, 10, 11, 12) need N % 128 == 0. */
int salun_gemm_bf16_supported(int64_t M, int N, int K);
int salun_gemm_bf16_nt(const void *x /*dev bf16*/, const void *w /*dev bf16*/, const float *bias /*dev or NULL*/,
                       const void *addend /*dev bf16 or NULL*/, void *y /*dev bf16*/, int64_t M, int N, int K,
                       int variant, salun_stream_t stream);
/* Weight gradient of the same layers (and of 1x1 stride-1 convolutions: salun_conv2d_bf16_backward_weight routes them
 * here):  dw[Na, Nb] fp32 (+= when accumulate) = dy[M, Na]^T . x[M, Nb]  (reference: autograd of F.linear / F.conv2d under
 * the layers above).  The reduction index M is the slow axis of both operands: tiles go global -> LDS directly and the
 * MFMA operands are gathered with transposing LDS reads.  Split over M into partials in `ws`
 * (salun_gemm_bf16_tn_workspace_bytes) folded in index order — deterministic.  Na, Nb multiples of 32, M < 2^24.
 * variant: 0 = choose (2); 1 = 128 x 128 tile, 64-token stages, 2 = 128 x 128, 32-token stages, 3 = 256 x 128, 64-token
 * stages (A/B measurements). */
int salun_gemm_bf16_tn_supported(int64_t M, int Na, int Nb);
size_t salun_gemm_bf16_tn_workspace_bytes(int64_t M, int Na, int Nb, int variant);
int salun_gemm_bf16_tn(const void *dy /*dev bf16*/, const void *x /*dev bf16*/, float *dw /*dev*/, int64_t M, int Na, int Nb,
                       int accumulate, int variant, void *ws /*dev or NULL*/, size_t ws_bytes, salun_stream_t stream);
/* The plan of salun_gemm_bf16_nt (op = SALUN_GEMM_BF16_NT; `ws_bytes` unused) or of salun_gemm_bf16_tn (op =
 * SALUN_GEMM_BF16_TN with (M, N, K) = (M, Na, Nb)) as a label, as salun_conv2d_bf16_route: host only; SALUN_OK or what the
 * entry point would return.  Labels: nt<WGM,WGN,db|sb>, nt_p<WGM,WGN>, nt_r<WGM,WGN,NST,BK>, tn<v<variant>>/S<split>. */
#define SALUN_GEMM_BF16_NT 0
#define SALUN_GEMM_BF16_TN 1
int salun_gemm_bf16_route(int op, int64_t M, int N, int K, int variant, size_t ws_bytes, char *buf, size_t buflen,
                          int *nsplit /*or NULL*/);
/* fp32 master weights w[N][K] -> the bf16 image the GEMM reads: [N][K] (transposed = 0) or [K][N] (transposed = 1).
 * Once per optimizer step per layer. */
int salun_pack_bf16(const float *w /*dev*/, void *wp /*dev bf16*/, int N, int K, int transposed, salun_stream_t stream);

/* Dropout whose keep decision is a function of (seed, GLOBAL element index) only — replaces
 * `nn.Dropout` in the DDPM ResnetBlock (DDPM/models/diffusion.py:108,124: `h = self.dropout(h)`), which under the
 * reference's nn.DataParallel draws independently per replica (runners/diffusion.py:504).
 *   gi   = (sample_offset + s) * chw + j                      global element index of sample s, position j
 *   bits = splitmix64(key + (gi >> 1)); even gi: bits >> 40, odd gi: (bits >> 8) & 0xFFFFFF
 *   y    = bits >= round(p * 2^24) ? x * (float)(1 / (1 - p)) : 0
 * key = seed + (seed_dev ? *seed_dev : 0)  (seed_dev: optional device word a captured graph advances with
 * salun_u64_add, so that replays draw fresh masks).  A rank holding samples [lo, hi) of a global batch passes
 * sample_offset = lo and gets rows lo..hi-1 of the single-process result; the backward pass is the same call on dy
 * (no mask is stored).  x, y: (n_samples, chw) fp32, y may alias x.  8 B / element. */
int salun_dropout(const float *x /*dev*/, float *y /*dev*/, int64_t n_samples, int64_t chw,
                  int64_t sample_offset, double p, uint64_t seed,
                  const uint64_t *seed_dev /*dev or NULL*/, salun_stream_t stream);
/* *value += inc on the stream (advances a device-resident seed between graph replays). */
int salun_u64_add(uint64_t *value /*dev*/, uint64_t inc, salun_stream_t stream);

/* ----------------------------------------------------------------- K17 --
 * IU / WoodFisher baseline (Classification/unlearn/Wfisher.py:47-198) from two scalars per retain sample,
 * a_i = <g_0, g_i> and b_i = <v, g_i>, computed from one batched eval-mode backward per batch
 * without materialising any per-sample gradient.  `out` (dev, B x 2 fp64, row-major: [i][0] for tangent 0 = g_0,
 * [i][1] for tangent 1 = v) is ACCUMULATED into, so one buffer collects every layer of a network.  All reductions
 * are fp64, per-workgroup partials in `ws` then a fixed-order finish: bit-identical from run to run, no atomics.
 * Workspace of the conv / BN dots: salun_iu_dot_workspace_bytes(B, n) with n = the per-sample element count.
 *
 * conv:    y2 (B, 2K, P, Q) = conv(x, [U_0; U_1]) (+ [u_b0; u_b1]);  dy (B, K, P, Q);  n = K*P*Q
 *          out[i][j] += sum_{c<n} y2[i][j*n + c] * dy[i][c]
 * BN eval: x, dy (B, C, HW);  out[i][j] += sum_{c,pq} dy * (ug_j[c] * (x - mean[c]) / sqrt(var[c] + eps) + ub_j[c])
 * linear:  x (B, K), dy (B, M), U_j (M, K), u_bj (M) or both NULL;  out[i][j] += sum_m dy[i][m] (U_j x_i + u_bj)[m]
 * B <= 65535 for the conv / BN dots. */
size_t salun_iu_dot_workspace_bytes(int B, int64_t n);
int salun_iu_conv_dot(const float *y2 /*dev*/, const float *dy /*dev*/, int B, int64_t n, double *out /*dev, B*2*/,
                      void *ws /*dev*/, size_t ws_bytes, salun_stream_t stream);
int salun_iu_bn_dot(const float *x /*dev*/, const float *dy /*dev*/, const float *running_mean /*dev, C*/,
                    const float *running_var /*dev, C*/, double eps, const float *u0_gamma /*dev, C*/,
                    const float *u0_beta /*dev, C*/, const float *u1_gamma /*dev, C*/, const float *u1_beta /*dev, C*/,
                    int B, int C, int HW, double *out /*dev, B*2*/, void *ws /*dev*/, size_t ws_bytes,
                    salun_stream_t stream);
int salun_iu_linear_dot(const float *x /*dev*/, const float *dy /*dev*/, const float *u0_w /*dev*/,
                        const float *u0_b /*dev or NULL*/, const float *u1_w /*dev*/, const float *u1_b /*dev or NULL*/,
                        int B, int M, int K, double *out /*dev, B*2*/, salun_stream_t stream);
/* The WoodFisher loop in scalar form, one thread in fp64:  s = 1, beta = 0;  for i < n (ab = (a_i, b_i) pairs of
 * samples 1 .. n of the reference's walk):  t = s a_i;  beta += (b_i - beta a_i) s / (N + t);  s *= N / (N + t).
 * out (dev, 2 fp64) = {beta, s}: the reference's k = v - beta g_0 and o = s g_0.  No host synchronisation. */
int salun_iu_recurrence(const double *ab /*dev, n*2*/, int64_t n, double N, double *out /*dev, 2*/,
                        salun_stream_t stream);
/* p[e] <- (float)((double)p[e] + alpha * ((double)v[e] - beta * (double)g0[e]))  where mask[e] != 0, everywhere
 * when mask is NULL; masked-out weights are not written.  beta: dev, 1 fp64 (salun_iu_recurrence's out[0]).
 * 16 B / element, 17 with a mask. */
int salun_iu_apply(float *p /*dev*/, const float *v /*dev*/, const float *g0 /*dev*/, const double *beta /*dev*/,
                   const uint8_t *mask /*dev or NULL*/, double alpha, int64_t n, salun_stream_t stream);

/* ----------------------------------------------------------------- K18 --
 * Fisher forgetting (`fisher_new`, Classification/unlearn/fisher.py:50-114).  The reference runs one
 * backward per class y and adds mean_i(prob[:, y]) * grad_y^2; in eval mode grad_y is linear in each layer's output
 * gradient, so all G class tangents come from one backward as a grouped dy [G*B, ...] over a shared input x [B, ...],
 * and F (dev fp32, ACCUMULATED into) gets sum_g w[g] * s_g^2 with s_g the complete group-g gradient.  Every group sum
 * is reduced to completion in a fixed order before it is squared; no float atomics: bit-identical from run to run.
 *
 * conv:   x (B, C, H, W), dy (G*B, K, P, Q), w (G), F (K, C, R, R): s_g = conv2d_backward_weight(x, dy_g) on the
 *         package's kernels (the shapes salun_conv2d_backward_weight takes; SALUN_EINVAL outside them).
 *         Workspace: salun_ff_conv_sq_workspace_bytes (0 = outside the domain).
 * linear: x (B, K), dy (G*B, M), F (M, K): s_g[m, k] = sum_{i<B} dy[g*B+i, m] x[i, k].
 * vector: dy (G*B, C, HW); F_beta[c] += sum_g w_g (sum_{i,pq} dy)^2 (conv / Linear bias, BN beta) and, when F_gamma is
 *         given, F_gamma[c] += sum_g w_g (sum dy (x - mean[c]) / sqrt(var[c] + eps))^2 with x (B, C, HW) (BN gamma).
 *         Workspace: salun_ff_vec_sq_workspace_bytes(G, C). */
size_t salun_ff_conv_sq_workspace_bytes(int G, int B, int C, int K, int R, int P, int Q);
int salun_ff_conv_sq(const float *x /*dev*/, const float *dy /*dev*/, const float *w /*dev, G*/, float *F /*dev*/,
                     int G, int B, int C, int H, int W, int K, int R, int stride, int pad, int P, int Q,
                     void *ws /*dev*/, size_t ws_bytes, salun_stream_t stream);
int salun_ff_linear_sq(const float *x /*dev*/, const float *dy /*dev*/, const float *w /*dev, G*/, float *F /*dev*/,
                       int G, int B, int M, int K, salun_stream_t stream);
size_t salun_ff_vec_sq_workspace_bytes(int G, int C);
int salun_ff_vec_sq(const float *x /*dev or NULL*/, const float *dy /*dev*/, const float *running_mean /*dev or NULL*/,
                    const float *running_var /*dev or NULL*/, double eps, const float *w /*dev, G*/, int G, int B,
                    int C, int HW, float *F_gamma /*dev or NULL*/, float *F_beta /*dev or NULL*/, void *ws /*dev*/,
                    size_t ws_bytes, salun_stream_t stream);
/* The reference's get_mean_var + p = mu + sqrt(var) z over the flat parameter arena, in place.  table (dev int64,
 * nparam rows of 7): offset, shape[0], shape[1] (1 for 1-D), prod(shape[2:]) (<= 256), flags (1: shape[0] ==
 * num_classes, 2: ndim > 1), the class row to override (-1: none), the parameter's first tile (a tile is one dim-0
 * row of a multi-dimensional parameter or 256 elements of a 1-D one; ntiles in all).  F is the raw sum of the batches'
 * grad2 terms: var = alpha * min(1 / (F / nbatches + 1e-8), 1e3 [, 1e2]); mean over dim 1 when ndim > 1; override row:
 * mu = 0, var = 1e-4; x10 when shape[0] == num_classes or ndim == 1.  z[e] is salun_fill_normal(seed, 0, 1)'s value at
 * the flat index e. */
int salun_ff_apply(float *p /*dev*/, const float *F /*dev*/, const int64_t *table /*dev*/, int nparam, int64_t ntiles,
                   double nbatches, double alpha, uint64_t seed, salun_stream_t stream);

/* Counter-based generators shared bit-for-bit with oracle/ (splitmix64 of
 * seed + index; integer arithmetic only, so CPU and GPU agree exactly):
 *   uniform: lo + (hi-lo) * (top 24 bits / 2^24);
 *   normal : mean + std * z, z = (sum of twelve 16-bit chunks of three
 *            splitmix64 outputs - 393210) / 65536  (Irwin-Hall 12: mean 0, var 1);
 *   u8     : byte (index & 7) of splitmix64(seed + (index >> 3)).
 * Used to regenerate identical synthetic inputs on any machine. */
int salun_fill_uniform(float *out /*dev*/, int64_t n, uint64_t seed, double lo, double hi,
                       salun_stream_t stream);
int salun_fill_normal(float *out /*dev*/, int64_t n, uint64_t seed, double mean, double std,
                      salun_stream_t stream);
int salun_fill_u8(uint8_t *out /*dev*/, int64_t n, uint64_t seed, salun_stream_t stream);

/* ----------------------------------------------------------------- K19 --
 * Sampling an (unlearned) CFG-DDPM (DDPM/sample.py).
 *
 * salun_sampler_step: one reverse step x_t -> x_next over a batch of B images of chw floats, fp32, one launch.
 *   e      = (1 + cond_scale) * eps_cond - cond_scale * eps_null        (eps_null NULL: e = eps_cond)
 *   at, an = abar[idx_t], abar[idx_next]   (the device table of alpha_bar_table: entry t + 1 is abar_t, entry 0 is 1;
 *            1 <= idx_t < table_len, 0 <= idx_next < table_len)
 *   SALUN_SAMPLER_ANCESTRAL:   beta = 1 - at / an;  x0 = clamp(sqrt(1 / at) x_t - sqrt(1 / at - 1) e, -1, 1);
 *            x_next = (sqrt(an) beta x0 + sqrt(1 - beta) (1 - an) x_t) / (1 - at) + sqrt(beta) z, no z at idx_t == 1
 *   SALUN_SAMPLER_GENERALIZED: x0 = (x_t - sqrt(1 - at) e) / sqrt(at);  c1 = eta sqrt((1 - at / an)(1 - an) / (1 - at));
 *            x_next = sqrt(an) x0 + c1 z + sqrt(1 - an - c1^2) e
 * with the coefficients computed on the device in the operation order of DDPM/functions/denoising.py.  z is `noise`
 * (dev, B * chw) when given; otherwise row b draws the counter-based normal of salun_fill_normal at element e of the
 * stream keyed by (seed, step, image_ids[b]) — the values salun_sampler_noise writes — so no noise tensor is read and
 * an image does not depend on the batch it is sampled in.  x0 (optional) receives the x0 estimate; x_next may be x_t. */
#define SALUN_SAMPLER_ANCESTRAL 0
#define SALUN_SAMPLER_GENERALIZED 1
int salun_sampler_step(const float *x_t /*dev*/, const float *eps_cond /*dev*/, const float *eps_null /*dev or NULL*/,
                       double cond_scale, const float *abar /*dev*/, int table_len, int idx_t, int idx_next, int variant,
                       double eta, const float *noise /*dev or NULL*/, uint64_t seed,
                       const int64_t *image_ids /*dev, B; may be NULL with noise*/, int64_t step, float *x_next /*dev*/,
                       float *x0 /*dev or NULL*/, int64_t B, int64_t chw, salun_stream_t stream);

/* out[b * chw + e] = salun_fill_normal(key(seed, step, image_ids[b]), 0, 1)[e] with
 * key = splitmix64(splitmix64(splitmix64(seed) + step) + image id): the start noise x_T (step 0) and, for tests, the
 * noise salun_sampler_step draws at a step. */
int salun_sampler_noise(float *out /*dev*/, uint64_t seed, const int64_t *image_ids /*dev, B*/, int64_t step, int64_t B,
                        int64_t chw, salun_stream_t stream);

/* lohi[0] = min x, lohi[1] = max x over n >= 1 floats: per-workgroup partials, then one workgroup, in a fixed order
 * (no float atomics). */
size_t salun_minmax_workspace_bytes(int64_t n);
int salun_minmax(const float *x /*dev*/, int64_t n, float *lohi /*dev, 2*/, void *ws /*dev*/, size_t ws_bytes,
                 salun_stream_t stream);

/* B images (C, HW) fp32 in the model's range -> uint8 (HW, C), one workgroup per image, C * HW <= 16000:
 *   v = clamp(rescaled ? (x + 1) / 2 : x, 0, 1);  u8 = trunc(clamp((clamp(v, lo, hi) - lo) / max(hi - lo, 1e-5) * 255 + 0.5, 0, 255))
 * `range` NULL: lo / hi are the image's own min / max of v.  Otherwise range[0..1] (dev) is a min / max of x values
 * (salun_minmax over all images of a grid), mapped like the pixels. */
int salun_images_to_u8(const float *x /*dev*/, uint8_t *out /*dev*/, int64_t B, int C, int HW, int rescaled,
                       const float *range /*dev, 2, or NULL*/, salun_stream_t stream);

/* ----------------------------------------------------------------- K21 --
 * The SD baselines (SD/train_scripts.py: train_esd; SD/ddim.py).
 *
 * salun_ldm_ddim_step: one reverse step of the LDM DDIM sampler on B latents of chw floats, fp32, one launch.
 *   guided != 0: eps2 is the output of ONE batched U-Net pass over cat([x, x]): rows [0, B) unconditional (e_u), rows
 *                [B, 2B) conditional (e_c), read in place;  e = e_u + scale * (e_c - e_u)
 *   guided == 0: eps2 holds B rows, e = eps2, and scale must be 1 (else SALUN_EINVAL)
 *   x0 = (x - c_s1m * e) / c_sqrt_at;  dir = c_dir * e;  x_prev = c_sqrt_aprev * x0 + dir [+ c_sigma * z]
 * Each step is one correctly rounded fp32 operation in this order (no contraction, IEEE division).  The coefficients are
 * fp32 values computed by the host from the DDIM tables (c_dir = sqrt(1 - a_prev - sigma^2)); the kernel recomputes
 * none.  c_sigma == 0: the noise term is skipped and z may be NULL; c_sigma != 0 with z == NULL is SALUN_EINVAL.
 * x0_out (optional) receives the x0 estimate; x_prev may be x.  Bound by launch latency at 4 x 64 x 64 latents. */
int salun_ldm_ddim_step(const float *x /*dev*/, const float *eps2 /*dev, 2B or B rows*/, int guided, double scale,
                        double c_s1m, double c_sqrt_at, double c_dir, double c_sqrt_aprev, double c_sigma,
                        const float *z /*dev or NULL*/, float *x_prev /*dev*/, float *x0_out /*dev or NULL*/, int64_t B,
                        int64_t chw, salun_stream_t stream);

/* The ESD objective and its gradient: e_0p is ONE batched frozen pass, rows [0, B) = e_0 (unconditional), rows
 * [B, 2B) = e_p (conditional); N = B * chw.
 *   target = e_0 - ng * (e_p - e_0);  loss = sum((e_n - target)^2) / N;  d_e_n = (2 / N) * (e_n - target)
 * target and d_e_n (both optional outputs) are sequences of correctly rounded fp32 operations; the sum folds fp32
 * squares in fp64 in a fixed order (partials per 1024-element segment, folded by one workgroup; no float atomics).  Up to
 * 64 segments — the workload's 4 x 64 x 64 latents are 16 — all of it is ONE launch of one workgroup; above, the
 * segments spread over the chip and a second launch folds, in the same order. */
size_t salun_esd_loss_workspace_bytes(int64_t B, int64_t chw);
int salun_esd_loss(const float *e_n /*dev*/, const float *e_0p /*dev, 2B rows*/, int64_t B, int64_t chw,
                   double negative_guidance, float *loss /*dev, 1*/, float *d_e_n /*dev or NULL*/,
                   float *target /*dev or NULL*/, void *ws /*dev*/, size_t ws_bytes, salun_stream_t stream);

/* ----------------------------------------------------------------- K22 --
 * Global unstructured pruning on the flat arena (csrc/salun_prune.hip).
 * Replaces  torch.nn.utils.prune.global_unstructured(L1Unstructured | RandomUnstructured)  over every nn.Conv2d weight
 *   Classification/pruner/utils.py:23-35,66-80  and the per-forward  weight_orig * weight_mask  of its hooks.
 * p (n floats) is the flat parameter vector, buf (n floats or NULL) the momentum vector, keep (n bytes, 1 = alive) the
 * prune mask.  segs (dev) holds nseg <= SALUN_PRUNE_MAX_SEGMENTS pairs (off, len) of disjoint ascending element ranges
 * of total length n_sel: the weights that may be pruned.  The kernels verify the table against n and n_sel before they
 * touch memory; a refused table changes nothing and is reported by salun_prune_status (error bit 2).
 * `alive` is the caller's count R of segment elements with keep == 1 (the host tracks it: n_sel at first, minus k_prune
 * per round); 0 <= k_prune <= alive.
 *   Among the alive segment elements the k_prune with the smallest |p| get keep = 0, p = 0, buf = 0.  Every other byte
 *   of p, buf and keep — outside the segments, already pruned, kept — is left bit-identical.  Ties at the threshold
 *   magnitude are pruned highest flat index first (the complement of K2's rule).  k_prune == 0 launches nothing,
 *   k_prune == alive prunes every alive element.  An alive weight of exactly 0.0 ranks by its magnitude like any other:
 *   pruned entries are told apart by keep, not by value, and never return.
 *   rnd (dev, n_sel floats, or NULL): rank by rnd[j] (j = position in the concatenated segments) instead of |p| — with
 *   salun_fill_uniform keys, a uniform draw without replacement among the alive weights.
 *   flags: SALUN_TOPK_FORCE_FULL_SCAN or 0.
 * Three launches: gather the keys (pruned entries as NaN, which K2 ranks after every number), salun_mask_topk_ex on the
 * compact keys with k = alive - k_prune, scatter.  Traffic: about 9 B per segment element plus the select's.
 * salun_prune_status synchronises the stream: `ranked` != 0 reads the select's status (route, error bit 1: its grid
 * barrier timed out and the round's result is INVALID) — pass it when 0 < k_prune < alive, the rounds that rank. */
#define SALUN_PRUNE_MAX_SEGMENTS 512
size_t salun_prune_workspace_bytes(int64_t n_sel);
int salun_prune_global(float *p /*dev*/, float *buf /*dev or NULL*/, uint8_t *keep /*dev*/, int64_t n,
                       const int64_t *segs /*dev, 2 * nseg*/, int nseg, int64_t n_sel, int64_t alive, int64_t k_prune,
                       const float *rnd /*dev or NULL*/, unsigned flags, void *ws /*dev*/, size_t ws_bytes,
                       salun_stream_t stream);
int salun_prune_status(const void *ws /*dev*/, int64_t n_sel, int ranked, int *route_out /*host*/,
                       int *error_out /*host*/, salun_stream_t stream);
/* *count (dev, 1 int64) = number of exact zeros (+0 or -0) of p inside the segments — check_sparsity's
 * torch.sum(weight == 0) over the conv layers — or -1 if the table was refused.  One memset and one launch, no sync. */
int salun_prune_count_zeros(const float *p /*dev*/, int64_t n, const int64_t *segs /*dev, 2 * nseg*/, int nseg,
                            int64_t n_sel, int64_t *count /*dev*/, salun_stream_t stream);

/* ----------------------------------------------------------------- K23 --
 * The fused classifier head (csrc/salun_cls_head.hip), fp32.
 * Replaces  AdaptiveAvgPool2d((1, 1)) -> flatten -> nn.Linear -> CrossEntropyLoss() -> utils.accuracy / AverageMeter
 *   Classification/models/ResNet.py:317-320, Classification/trainer/train.py:97-117  and their backward.
 * x [B, C, HW] (NCHW, contiguous), w [K, C], bias [K], labels [B] int64.
 *   pooled[b, c] = mean_hw x        logits[b, k] = bias[k] + sum_c pooled[b, c] w[k, c]
 *   p = softmax(logits) (maximum subtracted)          loss[b] = -log p[b, labels[b]]
 *   hit_b = (lowest index of the row's maximum == labels[b])
 * Forward: one memset (a 4-byte ticket in ws) and ONE launch.  It writes pooled, logits, p and loss[B], and — each
 * may be NULL — adds sum_b loss[b] (float64, fixed order) to *loss_sum, the number of hits to *hits and B to *count
 * (caller-owned running meters: no host synchronisation, no meter kernels), and writes the batch mean to *loss_mean.
 * ws is needed (salun_cls_head_workspace_bytes) when any of the four is given.
 * Backward: two launches.  scale = *grad_out / B (grad_out NULL: 1);
 *   dlogits[b, k] = (p[b, k] - [k == labels[b]]) * scale        dx[b, c, :] = (sum_k dlogits[b, k] w[k, c]) / HW
 *   dw[k, c] (+)= sum_b dlogits[b, k] pooled[b, c]               db[k] (+)= sum_b dlogits[b, k]
 * dx, dw, db may each be NULL (not computed); accumulate_w / accumulate_b != 0 add into dw / db.
 * A label outside [0, K) causes no out-of-range access: that sample's loss and its dlogits / dx rows are NaN, its hit
 * is 0, it counts in *count; the NaN reaches the sums (loss_sum, loss_mean, dw, db).
 * No floating-point atomics: every reduction has one order fixed by the shape, results are bit-identical run to run.
 * SALUN_EINVAL: B < 1, C outside [1, SALUN_CLS_HEAD_MAX_C], HW < 1, K outside [1, SALUN_CLS_HEAD_MAX_K] (the per-sample
 * rows live in LDS), a NULL required pointer, a pointer off its element's alignment (4 bytes; 8 for labels, loss_sum,
 * hits, count).  float4 loads / stores of x / dx are used when they are 16-byte aligned and HW % 4 == 0. */
#define SALUN_CLS_HEAD_MAX_C 8192
#define SALUN_CLS_HEAD_MAX_K 1024
size_t salun_cls_head_workspace_bytes(int64_t B, int C, int K);
int salun_cls_head_forward(const float *x /*dev*/, const float *w /*dev*/, const float *bias /*dev*/,
                           const int64_t *labels /*dev*/, float *pooled /*dev, B*C*/, float *logits /*dev, B*K*/,
                           float *p /*dev, B*K*/, float *loss /*dev, B*/, float *loss_mean /*dev, 1, or NULL*/,
                           double *loss_sum /*dev or NULL*/, int64_t *hits /*dev or NULL*/,
                           int64_t *count /*dev or NULL*/, int64_t B, int C, int HW, int K, void *ws /*dev*/,
                           size_t ws_bytes, salun_stream_t stream);
int salun_cls_head_backward(const float *p /*dev*/, const float *pooled /*dev*/, const float *w /*dev*/,
                            const int64_t *labels /*dev*/, const float *grad_out /*dev, 1, or NULL*/,
                            float *dlogits /*dev, B*K*/, float *dx /*dev or NULL*/, float *dw /*dev or NULL*/,
                            float *db /*dev or NULL*/, int accumulate_w, int accumulate_b, int64_t B, int C, int HW,
                            int K, salun_stream_t stream);

/* ----------------------------------------------------------------- K24 --
 * MaxPool2d(kernel_size=2, stride=2) of an fp32 NCHW tensor (csrc/salun_pool.hip).
 * Replaces  nn.MaxPool2d(kernel_size=2, stride=2)  Classification/models/VGG_LTH.py:86  and its backward.
 * x [NC, H, W] (contiguous; NC = batch * channels), y [NC, H/2, W/2], idx [NC, H/2, W/2] one byte per output:
 * the selected position inside the window, 0 top-left, 1 top-right, 2 bottom-left, 3 bottom-right.
 * Selection is that of torch.nn.functional.max_pool2d: scan in that order from (-inf, position 0), take a value
 * when it is greater than the running maximum or is NaN — the first of equal maxima wins, a later NaN replaces an
 * earlier one, +0 after -0 does not replace it.
 * Backward writes EVERY element of dx exactly once: the selected position gets the window's dy, the other three
 * +0.0.  One launch each, no atomics, no workspace; the same inputs give the same bits whatever the launch geometry.
 * 16-byte loads / stores (two outputs per item) are used when W % 4 == 0 and all three bases are 16-byte aligned,
 * one output per thread otherwise.  Indexing is 64-bit.
 * SALUN_EINVAL (nothing is written): NC < 1, H or W odd or < 2, a NULL pointer, a float pointer off 4-byte
 * alignment, dx == dy. */
int salun_maxpool2x2_forward(const float *x /*dev*/, float *y /*dev, NC*H/2*W/2*/, uint8_t *idx /*dev, NC*H/2*W/2*/,
                             int64_t NC, int H, int W, salun_stream_t stream);
int salun_maxpool2x2_backward(const float *dy /*dev*/, const uint8_t *idx /*dev*/, float *dx /*dev, NC*H*W*/,
                              int64_t NC, int H, int W, salun_stream_t stream);

/* ----------------------------------------------------------------- K25 --
 * RBF C-SVC fit and predict for the membership-inference attack (csrc/salun_svc.hip).
 * Replaces  sklearn.svm.SVC(C=3, gamma='auto', kernel='rbf').fit / .predict  Classification/evaluation/SVC_MIA.py:53-82.
 * The problem is libsvm's C-SVC dual (Fan, Chen, Lin 2005):  min 1/2 a'Qa - e'a,  0 <= a_t <= C,  y'a = 0,
 *   Q_ts = y_t y_s K_ts,  K_ts = exp(-gamma |x_t - x_s|^2),  y_t = +1 where y01[t] != 0 (member), -1 otherwise,
 *   f(z) = sum_t a_t y_t K(x_t, z) - rho,  member iff f(z) > 0.
 * X [n, d] fp32 row-major, 2 <= n <= SALUN_SVC_MAX_N, 1 <= d <= SALUN_SVC_MAX_D.
 * ws (salun_svc_rbf_workspace_bytes(n), 0 outside the limits): K [n, n] fp32, then the solver's gradient and state.
 * salun_svc_rbf_gram: K_ts into ws, all CUs.  The squared distance is summed over the features in index order in
 *   fp64, multiplied by -gamma, exp in fp64, and the entry rounded ONCE to fp32 (libsvm's Qfloat).
 * salun_svc_rbf_fit: SMO on the K that salun_svc_rbf_gram left in ws (same ws, same n): second-order working-set
 *   selection (WSS 2), no shrinking; alpha, gradient and rho in fp64; ties in either selection go to the lowest
 *   index; a curvature <= 0 is replaced by 1e-12; libsvm's clipped two-variable update (a clipped value IS 0 or C);
 *   stops when m(alpha) - M(alpha) < eps or after max_iter updates; rho = mean of y_t G_t over free variables, else the
 *   midpoint of the bounds.  ONE launch of ONE workgroup runs the whole loop: no grid barrier, no cross-workgroup
 *   flag, no spin; the loop is bounded by max_iter.  Writes alpha[n], *rho and status[0] = updates made,
 *   status[1] = 1 if the stopping rule was met, 0 if max_iter ended the loop (alpha is feasible either way).
 *   Deterministic: the same inputs give the same bits.
 * salun_svc_rbf_decision: dec[q] = sum_t coef[t] K(x_t, z_q) - *rho in fp64 over the entries with coef[t] != 0
 *   (coef[t] = alpha_t y_t), fixed summation order, and pred[q] = (dec[q] > 0).  dec or pred may be NULL.  All CUs.
 * SALUN_EINVAL: n, d or m outside the limits, a NULL required pointer, C <= 0, eps <= 0, gamma <= 0 or not finite,
 *   max_iter < 0.  SALUN_ENOSPC: ws_bytes short of the query.
 * salun_svc_rbf_gram_wide / salun_svc_rbf_decision_wide: the same contracts for 1 <= d <= SALUN_SVC_WIDE_MAX_D (the
 *   attack's probability-vector feature has one entry per class: 100 for CIFAR-100, 200 for Tiny-ImageNet).  The
 *   feature rows and the query point pass through LDS instead of registers; the arithmetic and its order are those
 *   of the narrow pair, so for d <= SALUN_SVC_MAX_D the results are the same bits.  salun_svc_rbf_fit serves both. */
#define SALUN_SVC_MAX_N 65536
#define SALUN_SVC_MAX_D 16
#define SALUN_SVC_WIDE_MAX_D 1024
size_t salun_svc_rbf_workspace_bytes(int64_t n);
int salun_svc_rbf_gram(const float *X /*dev, n*d*/, int64_t n, int d, double gamma, void *ws /*dev*/, size_t ws_bytes,
                       salun_stream_t stream);
int salun_svc_rbf_fit(const uint8_t *y01 /*dev, n*/, int64_t n, double C, double eps, int64_t max_iter,
                      double *alpha /*dev, n*/, double *rho /*dev, 1*/, int64_t *status /*dev, 2*/, void *ws /*dev*/,
                      size_t ws_bytes, salun_stream_t stream);
int salun_svc_rbf_decision(const float *X /*dev, n*d*/, const double *coef /*dev, n*/, const double *rho /*dev, 1*/,
                           int64_t n, int d, double gamma, const float *Z /*dev, m*d*/, int64_t m,
                           double *dec /*dev, m, or NULL*/, uint8_t *pred /*dev, m, or NULL*/, salun_stream_t stream);
int salun_svc_rbf_gram_wide(const float *X /*dev, n*d*/, int64_t n, int d, double gamma, void *ws /*dev*/,
                            size_t ws_bytes, salun_stream_t stream);
int salun_svc_rbf_decision_wide(const float *X /*dev, n*d*/, const double *coef /*dev, n*/,
                                const double *rho /*dev, 1*/, int64_t n, int d, double gamma,
                                const float *Z /*dev, m*d*/, int64_t m, double *dec /*dev, m, or NULL*/,
                                uint8_t *pred /*dev, m, or NULL*/, salun_stream_t stream);

/* ----------------------------------------------------------------- K26 --
 * Antialiased bilinear resample of uint8 images, bit-identical to Pillow's 8-bit path (csrc/salun_resample.hip;
 * DESIGN.md §9l).  Replaces  transforms.Resize(config.data.image_size)  DDPM/datasets/__init__.py:36-41, i.e.
 * PIL.Image.resize((OW, OH), Image.BILINEAR), which the reference runs on the host for every fetch.
 * src [B, H, W, C] uint8, dst [B, OH, OW, C] uint8, both contiguous, any byte alignment; B >= 1, C in {1, 3, 4},
 * 1 <= H, W, OH, OW <= SALUN_RESAMPLE_MAX_SIDE.
 * Per axis (in source samples, out destination samples):  scale = in / out, fs = max(scale, 1), support = 1.0 * fs,
 *   ss = 1 / fs;  for output index xx:  center = (xx + 0.5) * scale,  xmin = max(0, (int)(center - support + 0.5)),
 *   xmax = min(in, (int)(center + support + 0.5)),  taps x in [0, xmax - xmin) with
 *   w = max(0, 1 - |(x + xmin - center + 0.5) * ss|), divided by their sum, then k = (int)(w * 2^22 + 0.5).
 * An output byte is clip8((2^21 + sum k * pixel) >> 22); the horizontal pass runs first and is rounded to uint8 before
 * the vertical pass reads it.  The tables are computed on the host in doubles (no contraction to fused multiply-adds),
 * uploaded once per (device, in, out) pair and kept; the first call for a pair blocks the host for that copy.
 * ONE launch: a workgroup produces a band of output rows of one image; the horizontal result of the source rows the
 * band needs lives in LDS and never reaches memory.  salun_resample_u8_lds_bytes is that LDS size for the band height
 * the launch would use (host arithmetic only), 0 when the arguments are outside the limits or when a band of ONE
 * output row would need more than SALUN_RESAMPLE_MAX_LDS bytes — such a call is refused, nothing is spilled.
 * salun_resample_u8_table copies ONE axis's table to HOST memory (no device call; what the tests compare with their
 * restatement): out first-tap indices, out tap counts, then out rows of *ksize weights (unused tail 0), i.e.
 * out * (2 + *ksize) int32.  table == NULL only reports *ksize; SALUN_ENOSPC when n_ints is short.
 * SALUN_EINVAL (nothing is written): any limit above, a NULL pointer, dst == src, a refused size pair. */
#define SALUN_RESAMPLE_MAX_SIDE 1024
#define SALUN_RESAMPLE_MAX_LDS 65536
size_t salun_resample_u8_lds_bytes(int H, int W, int C, int OH, int OW);
int salun_resample_u8_table(int in, int out, int32_t *table /*host, or NULL*/, size_t n_ints, int *ksize /*host*/);
int salun_resample_u8(const uint8_t *src /*dev, B*H*W*C*/, uint8_t *dst /*dev, B*OH*OW*C*/, int64_t B, int H, int W,
                      int C, int OH, int OW, salun_stream_t stream);

/* ----------------------------------------------------------------- K27 --
 * Forward-only fp32 convolution for arbitrary map sizes with the epilogue of a folded BatchNorm
 * (csrc/salun_conv_infer.hip), and the three small kernels the classifier evaluation needs around it.
 * Replaces, in eval mode,  torchvision.models.resnet34(...)  DDPM/classifier_evaluation.py:135-143  layer by layer:
 * nn.Conv2d(bias=False) -> nn.BatchNorm2d (running statistics) [-> + identity] [-> ReLU].
 *   y[n,k,p,q] = act( conv(x, w)[n,k,p,q] * scale[k] + shift[k] + addend[n,k,p,q] )
 * x [N, C, H, W], w [K, C, R, R] (OIHW, read in place), y and addend [N, K, P, Q], scale and shift [K]; scale, shift and
 * addend may each be NULL (the term is skipped); relu != 0: act(o) = o < 0 ? 0 : o (a NaN stays a NaN).  `pad` is the
 * low-side padding; P and Q are the caller's.  The epilogue operations are applied in the order written, each rounded by
 * itself (no fused multiply-add).  The reduction is an exact-fp32 FMA chain on v_mfma_f32_32x32x2_f32 as in K8.
 * Domain: R in {1, 3, 7}; stride in {1, 2}; 0 <= pad < R; K a multiple of 32 (<= 65536); 1 <= C <= 65536, a multiple
 * of 8 unless R == 7; 1 <= H, W, P, Q <= 1024 with the first tap of the last output row / column inside the padded
 * input ((P - 1) stride - pad < H, likewise Q); N >= 1, N P Q <= 2^40.  N P Q need not fill a tile: the last pixel
 * tile is masked.  Indexing is 64-bit.
 * `tile`: SALUN_INFER_TILE_AUTO picks pixels x channels from the problem (the largest of 128x128, 128x64, 64x64 that
 * still gives every CU a workgroup); the other values force one (tests, tuning).  Every tile gives the same bits.
 * One launch, no workspace, no atomics: the same inputs give the same bits, and an image's output does not depend on
 * the rest of the batch.
 * SALUN_EINVAL (nothing is written): anything outside the domain, a NULL x, w or y, addend == y, x == y, a pointer off
 * 4-byte alignment.
 * salun_conv2d_infer_route: the label of the plan the call would run, from the plan function the launch uses; touches
 * no device.  infer<R,stride>/<pixels>x<channels>/<fast|generic>/B<workgroups>; fast: C % 16 == 0 (tap-outermost
 * reduction), generic: any C (OIHW-order reduction, zero-padded to a multiple of 16).  SALUN_ENOSPC: buf too short. */
#define SALUN_INFER_TILE_AUTO 0
#define SALUN_INFER_TILE_64X64 1
#define SALUN_INFER_TILE_128X64 2
#define SALUN_INFER_TILE_128X128 3
int salun_conv2d_infer(const float *x /*dev*/, const float *w /*dev*/, const float *scale /*dev, K, or NULL*/,
                       const float *shift /*dev, K, or NULL*/, const float *addend /*dev, N*K*P*Q, or NULL*/,
                       float *y /*dev, N*K*P*Q*/, int N, int C, int H, int W, int K, int R, int stride, int pad, int P,
                       int Q, int relu, int tile, salun_stream_t stream);
int salun_conv2d_infer_route(int N, int C, int H, int W, int K, int R, int stride, int pad, int P, int Q, int tile,
                             char *buf, size_t buflen);

/* K27 with a nearest-neighbour 2x input: the decoder's Upsample in one launch.
 * Replaces  torch.nn.functional.interpolate(x, scale_factor=2.0, mode="nearest")  followed by  self.conv  (3 x 3,
 * stride 1, padding 1) in  Upsample.forward  (ldm/modules/diffusionmodules/model.py:53-57).
 *   y = act( conv(up2(x), w) * scale[k] + shift[k] + addend ),   up2(x)[n,c,i,j] = x[n,c,i>>1,j>>1]
 * up2(x) is the VIRTUAL [N, C, 2H, 2W] map: it is never written.  H and W are the STORED sizes of x; P, Q, pad, the
 * epilogue, the reduction order and the tiles are those of salun_conv2d_infer applied to the virtual map, so the bits
 * equal those of salun_conv2d_infer on the materialised up2(x) with the same tile.  The halo test is made in virtual
 * coordinates (0 <= ih < 2H) before the shift: a tap at virtual row -1 or 2H contributes zero.
 * Domain: that of salun_conv2d_infer on (N, C, 2H, 2W, K, R, stride, pad, P, Q), narrowed to R == 3, stride == 1,
 * C a multiple of 8, 1 <= H, W <= 512.  Both reduction orders and all three tiles are served.
 * SALUN_EINVAL (nothing is written): as salun_conv2d_infer.
 * salun_conv2d_infer_up2_route: the plain label with `^2` after the filter:
 * infer<3,1>^2/<pixels>x<channels>/<fast|generic>/B<workgroups>. */
int salun_conv2d_infer_up2(const float *x /*dev, N*C*H*W*/, const float *w /*dev*/,
                           const float *scale /*dev, K, or NULL*/, const float *shift /*dev, K, or NULL*/,
                           const float *addend /*dev, N*K*P*Q, or NULL*/, float *y /*dev, N*K*P*Q*/, int N, int C, int H,
                           int W, int K, int R, int stride, int pad, int P, int Q, int relu, int tile,
                           salun_stream_t stream);
int salun_conv2d_infer_up2_route(int N, int C, int H, int W, int K, int R, int stride, int pad, int P, int Q, int tile,
                                 char *buf, size_t buflen);

/* ----------------------------------------------------------------- K30 --
 * Forward-only fp32 POINTWISE convolution (1 x 1, stride 1, no padding) with K27's epilogue
 * (csrc/salun_conv1x1_infer.hip).  Replaces, in eval mode, the conv1 / conv3 / stride-1 downsample
 * convolutions of  torchvision.models.resnet50  (SD/eval-scripts/imageclassify.py:24-26)  with their BatchNorm,
 * residual add and ReLU.
 *   y[n,k,g] = act( (sum_c w[k,c] x[n,c,g]) * scale[k] + shift[k] + addend[n,k,g] ),   g in [0, HW)
 * x [N, C, HW], w [K, C], y and addend [N, K, HW], scale and shift [K]; scale, shift and addend may each be NULL; relu
 * and the epilogue (each operation rounded by itself, in the order written) are salun_conv2d_infer's.
 * Reduction: ONE fp32 FMA chain per output element over c in ascending order on v_mfma_f32_32x32x2_f32, no split over
 * C - the chain salun_conv2d_infer runs for R == 1, so the two return the same bits and a caller may route a layer to
 * either.  (A reduction tail is padded with (+0)(+0) products, as K27's generic order pads.)
 * Domain: N >= 1, HW >= 1, N HW <= 2^40; C a multiple of 8, 8 <= C <= 65536; K a multiple of 32, 32 <= K <= 65536.
 * Indexing is 64-bit.  Tiles span images; the last pixel tile and a channel tile K does not fill are masked.
 * Staging: x is read as 16-byte row segments where HW % 4 == 0 and x and y are 16-byte aligned, else 4 bytes at a
 * time; w as 16-byte segments where w is 16-byte aligned.  Every path gives the same bits.
 * `tile`: SALUN_INFER_TILE_*, as salun_conv2d_infer (same AUTO rule); every tile gives the same bits.
 * One launch, no workspace, no atomics: the same inputs give the same bits, and an image's output does not depend on
 * the rest of the batch.
 * SALUN_EINVAL (nothing is written): anything outside the domain, a NULL x, w or y, addend == y, x == y, a pointer off
 * 4-byte alignment.
 * salun_conv1x1_infer_route: the label of the plan a call would run, from the plan function the launch uses; touches
 * no device.  aligned16: x and y are 16-byte aligned; w_aligned16: w is.
 * pw/<pixels>x<channels>/<vec16|vec4|scalar>/B<workgroups>; vec16: 16-byte loads of x and w, vec4: 4-byte loads of x,
 * scalar: 4-byte loads of both.  SALUN_ENOSPC: buf too short. */
int salun_conv1x1_infer(const float *x /*dev, N*C*HW*/, const float *w /*dev, K*C*/,
                        const float *scale /*dev, K, or NULL*/, const float *shift /*dev, K, or NULL*/,
                        const float *addend /*dev, N*K*HW, or NULL*/, float *y /*dev, N*K*HW*/, int N, int C, int64_t HW,
                        int K, int relu, int tile, salun_stream_t stream);
int salun_conv1x1_infer_route(int N, int C, int64_t HW, int K, int tile, int aligned16, int w_aligned16, char *buf,
                              size_t buflen);

/* MaxPool2d(kernel_size=3, stride=2, padding=1), forward only (csrc/salun_pool.hip, beside K24).
 * Replaces  resnet34().maxpool  (DDPM/classifier_evaluation.py:135).
 * x [NC, H, W] (contiguous), y [NC, (H+1)/2, (W+1)/2], any H, W >= 1.  Padding acts as -inf.  Selection is that of
 * torch.nn.functional.max_pool2d: scan the window row by row, left to right, from -inf and take a value when it is
 * greater than the running maximum or is NaN - the first of equal maxima wins, a NaN wins, +0 after -0 does not
 * replace it.  One launch, one output per thread, 64-bit indexing.
 * SALUN_EINVAL (nothing is written): NC < 1, H or W < 1 or > 2^20, a NULL pointer, y == x, a pointer off 4-byte
 * alignment. */
int salun_maxpool3x3s2_forward(const float *x /*dev*/, float *y /*dev, NC*((H+1)/2)*((W+1)/2)*/, int64_t NC, int H,
                               int W, salun_stream_t stream);

/* transforms.ToTensor() + transforms.Normalize(mean, std) of uint8 images (csrc/salun_imgnorm.hip).
 * Replaces  DDPM/classifier_evaluation.py:94-100  (after the Resize, which is K26).
 * src [B, H, W, C] uint8 (K26's output layout), dst [B, C, H, W] fp32:
 *   dst[b,c,h,w] = ((float(src[b,h,w,c]) / 255) - mean[c]) / std[c],  every step rounded to fp32 - bit for bit what
 * torch computes.  salun_u8_norm_table fills the 256 x C table of that expression in HOST memory (table[c * 256 + u];
 * host arithmetic, no device call); the caller uploads it once and passes the device copy to salun_u8_to_chw_norm.
 * SALUN_EINVAL (nothing is written): B, H or W < 1, C outside [1, SALUN_U8_NORM_MAX_C], a NULL pointer, table or dst
 * off 4-byte alignment. */
#define SALUN_U8_NORM_MAX_C 4
int salun_u8_norm_table(const float *mean /*host, C*/, const float *std /*host, C*/, int C, float *table /*host, 256*C*/);
int salun_u8_to_chw_norm(const uint8_t *src /*dev, B*H*W*C*/, const float *table /*dev, 256*C*/,
                         float *dst /*dev, B*C*H*W*/, int64_t B, int H, int W, int C, salun_stream_t stream);

/* salun_u8_to_chw_norm of a WINDOW of the source: transforms.CenterCrop then ToTensor + Normalize without a copy of the
 * crop.  Replaces the crop and normalise of  ResNet50_Weights.DEFAULT.transforms()  (SD/eval-scripts/imageclassify.py:27).
 * src [B, H, W, C] uint8, dst [B, C, OH, OW] fp32:  dst[b,c,i,j] = table[c][src[b, top + i, left + j, c]], the table of
 * salun_u8_norm_table.  With top == left == 0, OH == H, OW == W it writes what salun_u8_to_chw_norm writes.
 * SALUN_EINVAL (nothing is written): as salun_u8_to_chw_norm; a window that does not lie inside the image (top or
 * left < 0, OH or OW < 1, top + OH > H, left + OW > W). */
int salun_u8_crop_to_chw_norm(const uint8_t *src /*dev, B*H*W*C*/, const float *table /*dev, 256*C*/,
                              float *dst /*dev, B*C*OH*OW*/, int64_t B, int H, int W, int C, int top, int left, int OH,
                              int OW, salun_stream_t stream);

/* The evaluation head (csrc/salun_cls_head.hip, beside K23): pool -> fc -> softmax as salun_cls_head_forward (same
 * statements, same rounding points), then the figures of DDPM/classifier_evaluation.py:22-36 for ONE label shared by
 * the whole batch.  Replaces  model.avgpool / model.fc  and  validate()'s  argmax / softmax / log / sums.
 * Writes logits [B, K] and p [B, K] and ADDS to caller-owned device meters (each may be NULL; no host synchronisation):
 *   *entropy_sum (float64) += sum_b -(sum_k p[b,k] * logf(p[b,k]))      *prob_sum (float64) += sum_b p[b, label]
 *   *hits (int64) += #{b : lowest index of the row's maximum == label}  *count (int64) += B
 * zero_safe == 0: every entropy term is the reference's fp32 expression p * log(p); a probability that underflowed
 * to 0 gives 0 * -inf = NaN for the sample and the sum, as the reference does.  zero_safe != 0: such a term is 0.
 * The per-sample values are folded in float64 in one fixed order by the last workgroup to finish (a ticket in ws, cleared
 * by a memset ahead of the ONE launch); no floating-point atomics: the same inputs give the same bits.
 * ws: salun_cls_head_eval_workspace_bytes(B, C, K) bytes (0: outside the limits).
 * SALUN_EINVAL: the limits of salun_cls_head_forward, label outside [0, K), a NULL x, w, bias, logits, p or ws, a
 * pointer off its element's alignment.  SALUN_ENOSPC: ws_bytes short of the query. */
size_t salun_cls_head_eval_workspace_bytes(int64_t B, int C, int K);
int salun_cls_head_eval(const float *x /*dev, B*C*HW*/, const float *w /*dev, K*C*/, const float *bias /*dev, K*/,
                        int label, float *logits /*dev, B*K*/, float *p /*dev, B*K*/,
                        double *entropy_sum /*dev or NULL*/, double *prob_sum /*dev or NULL*/,
                        int64_t *hits /*dev or NULL*/, int64_t *count /*dev or NULL*/, int64_t B, int C, int HW, int K,
                        int zero_safe, void *ws /*dev*/, size_t ws_bytes, salun_stream_t stream);

/* The k largest entries of every row, sorted, with their indices (csrc/salun_row_topk.hip).
 * Replaces  torch.topk(probs, topk)  (SD/eval-scripts/imageclassify.py:66) on the p of salun_cls_head_eval.
 * p [B, K] fp32, values [B, k] fp32 (the entries' own bits), indices [B, k] int64; 1 <= K <= SALUN_CLS_HEAD_MAX_K,
 * 1 <= k <= K, 1 <= B < 2^31.
 * THE ORDER: a larger value comes first; a NaN ranks above every number; equal values - NaNs among themselves and -0
 * with +0 included - go by ascending index.  That is torch.topk's result wherever a row has no ties; on ties torch
 * promises nothing and this does.
 * One launch, one workgroup per row, no atomics, no workspace: deterministic.
 * SALUN_EINVAL (nothing is written): a size outside the limits, a NULL pointer, a pointer off its element's alignment. */
int salun_row_topk(const float *p /*dev, B*K*/, float *values /*dev, B*k*/, int64_t *indices /*dev, B*k*/, int64_t B,
                   int K, int k, salun_stream_t stream);

/* ----------------------------------------------------------------- K28 --
 * GroupNorm (+ SiLU) forward for groups too large for one workgroup (csrc/salun_gn_split.hip).
 * Replaces  Normalize(in_channels) = torch.nn.GroupNorm(32, C, eps=1e-6, affine=True)  followed by  nonlinearity(x) =
 * x * sigmoid(x)  in ldm/modules/diffusionmodules/model.py:33-39 (ResnetBlock, AttnBlock, Encoder.norm_out), at the
 * map sizes of the first-stage encoder, where salun_gn_forward refuses (H W not a power of two, cpg HW > 262144).
 *   y = [silu](gamma[c] * (x - mean[n,g]) * rstd[n,g] + beta[c]),  x and y [N, C, HW], statistics over the cpg * HW
 * contiguous values of an (image, group), biased variance.  The arithmetic is salun_gn_forward's, statement for
 * statement: lanes add float4 trees in fp32 and fold into doubles every SALUN_GN_SPLIT_FLUSH float4s; block sums, the
 * fold of the slabs, mean and variance are in double; a = rstd * gamma[c], b = beta[c] - mean * a, o = x * a + b, each
 * rounded by itself; SiLU is o * (1 / (1 + expf(-o))).
 * A group is cut into S = ceil(cpg HW / 4 / slab) slabs of `slab` float4s (the last may be shorter; a boundary may fall
 * inside a channel or between channels).  Two launches over a grid of N G S, no atomics: the first writes one (sum, sum
 * of squares) pair of doubles per slab to ws, the second folds a group's S pairs in index order in every workgroup of
 * the group, writes save_mean / save_rstd [N * G] from slab 0 and applies over its slab.
 * slab_vec4 == 0: slab = 2048 float4s (8 per lane).  S depends on cpg HW and slab_vec4 only - not on N, not on the
 * device - so the same inputs give the same bits and an image's output does not depend on the rest of the batch.
 * Any other slab_vec4 > 0 forces the slab length (tests, tuning).
 * Domain: N, G >= 1, C % G == 0, HW >= 4 and a multiple of 4, cpg HW < 2^31, N G S < 2^31; x and y 16-byte aligned;
 * y == x is allowed (an element is read before it is written, the statistics are complete by then).
 * SALUN_EINVAL (nothing is written): anything outside the domain, slab_vec4 < 0, a NULL pointer, ws off 8-byte
 * alignment or ws_bytes short of salun_gn_split_workspace_bytes (0 outside the domain).
 * salun_gn_split_slabs: S (0 outside the domain); touches no device. */
#define SALUN_GN_SPLIT_FLUSH 16
size_t salun_gn_split_workspace_bytes(int N, int C, int64_t HW, int G, int slab_vec4);
int salun_gn_split_slabs(int C, int64_t HW, int G, int slab_vec4);
int salun_gn_split_forward(const float *x /*dev*/, float *y /*dev*/, const float *gamma /*dev, C*/,
                           const float *beta /*dev, C*/, float *save_mean /*dev, N*G*/, float *save_rstd /*dev, N*G*/,
                           int N, int C, int64_t HW, int G, double eps, int silu, int slab_vec4, void *ws /*dev*/,
                           size_t ws_bytes, salun_stream_t stream);

/* The posterior of the first stage (csrc/salun_vae.hip).  Replaces  DiagonalGaussianDistribution.sample() / .mode()
 * (ldm/modules/distributions/distributions.py:24-45) and the  scale_factor *  of get_first_stage_encoding
 * (ldm/models/diffusion/ddpm.py:535-543).
 * moments [B, Cm, hw] with Cm >= 2 zc: channels [0, zc) are the mean, [zc, 2 zc) the log-variance, further channels are
 * ignored (the output of a convolution whose K was zero-padded is read in place).  z [B, zc, hw]:
 *   z = scale * (mean + expf(0.5 * clamp(logvar, -30, 20)) * e),   deterministic != 0: z = scale * mean,
 * every operation rounded by itself, scale rounded to fp32 first.  e is the value salun_sampler_noise(seed, image_ids,
 * step = draw, chw = zc * hw) writes at the element's index c * hw + p: an image's latent does not depend on where it
 * sits in a batch, and another `draw` gives an independent one.
 * SALUN_EINVAL (nothing is written): zc, hw or B < 1, Cm < 2 zc, draw < 0, B Cm hw > 2^40, a NULL moments or z, NULL
 * image_ids unless deterministic, moments == z, a pointer off 4-byte alignment. */
int salun_vae_posterior_sample(const float *moments /*dev, B*Cm*hw*/, int Cm, int zc, int64_t hw, int64_t B,
                               const int64_t *image_ids /*dev, B*/, uint64_t seed, int64_t draw, double scale,
                               int deterministic, float *z /*dev, B*zc*hw*/, salun_stream_t stream);

/* The decoded image as bytes (csrc/salun_vae.hip).  Replaces  image = (image / 2 + 0.5).clamp(0, 1);
 * image.permute(0, 2, 3, 1).numpy();  (image * 255).round().astype("uint8")  of SD/eval-scripts/generate-images.py.
 * x [B, Cp, hw] fp32, out [B, hw, C] uint8, 1 <= C <= min(Cp, SALUN_DECODED_U8_MAX_C): the first C of Cp planes are read,
 * so the channel-padded output of the decoder's conv_out is read in place.  Per element, every operation rounded by
 * itself:  v = x * 0.5f;  v = v + 0.5f;  v = min(max(v, 0), 1);  v = v * 255.f;  u8 = rintf(v)  (half to even, as
 * numpy's round).  A NaN gives 0.  Any hw; 64-bit indexing.  salun_images_to_u8 is another rule and stays.
 * SALUN_EINVAL (nothing is written): B or hw < 1, C outside its range, B Cp hw > 2^40, a NULL pointer, x == out, x off
 * 4-byte alignment. */
#define SALUN_DECODED_U8_MAX_C 4
int salun_decoded_to_u8(const float *x /*dev, B*Cp*hw*/, int Cp, int C, int64_t hw, int64_t B,
                        uint8_t *out /*dev, B*hw*C*/, salun_stream_t stream);

/* One step of the linear multistep (LMS) sampler of the evaluation script on B latents of chw floats, one launch
 * (csrc/salun_sampler.hip; SD/lms.py computes the coefficients on the host in float64).
 *   guided != 0: eps2 is ONE batched U-Net pass, rows [0, B) unconditional (e_u), rows [B, 2B) conditional (e_c), read
 *                in place;  d = e_u + scale * (e_c - e_u)
 *   guided == 0: eps2 holds B rows, d = eps2, and scale must be 1 (else SALUN_EINVAL)
 *   hist[slot] = d                                  (hist: a ring of SALUN_LMS_ORDER rows of B * chw floats)
 *   a = x + c[0] * d;  a = a + c[j] * hist[(slot - j) mod SALUN_LMS_ORDER]  for j = 1 .. order - 1, in that order
 *   x_new = a;   x_in[r] = a / den  for r = 0 (and r = 1 when guided): the [2B, chw] or [B, chw] input of the next pass
 * Every operation is one correctly rounded fp32 operation (no contraction, IEEE division); c[] and den are rounded to
 * fp32 first; den = sqrt(sigma_next^2 + 1) is the host's value.  x_new may be x; x_in may be NULL.
 * SALUN_EINVAL (nothing is written): order outside [1, SALUN_LMS_ORDER], slot outside [0, SALUN_LMS_ORDER), B or chw
 * < 0, den == 0, a NULL x, eps2, hist or x_new, hist or x_in equal to another argument. */
#define SALUN_LMS_ORDER 4
int salun_lms_step(const float *x /*dev*/, const float *eps2 /*dev, 2B or B rows*/, int guided, double scale,
                   float *hist /*dev, SALUN_LMS_ORDER*B*chw*/, int slot, int order, double c0, double c1, double c2,
                   double c3, double den, float *x_new /*dev*/, float *x_in /*dev, 2B or B rows, or NULL*/, int64_t B,
                   int64_t chw, salun_stream_t stream);

/* ----------------------------------------------------------------- K29 --
 * The CLIP text encoder of Stable Diffusion v1 (csrc/salun_clip_text.hip).  Replaces, together with the
 * K15 GEMM for the Linear layers, transformers' CLIPTextModel as SD/ldm/modules/encoders/modules.py
 * `FrozenCLIPEmbedder.forward` calls it.  All four are fp32, forward only and deterministic; the rounding points of each
 * are listed in the header comment of the source file.
 *
 * salun_clip_embed: x[b, t, :] = tok[ids[b, t], :] + pos[t, :] for ids [B, T] (int64), tok [V, W], pos [>= T, W]: one
 * fp32 add per element.  The caller validates the ids (they come from the host tokenizer); an id outside [0, V) reads
 * nothing and writes a row of NaN.
 * SALUN_EINVAL (nothing is written): B or T < 1, W < 4 or no multiple of 4, V < 1, a NULL pointer, tok, pos or x off
 * 16-byte alignment, ids off 8-byte alignment.
 *
 * salun_ln_f32_forward: y = (x - mean) / sqrt(var + eps) * gamma + beta over the last dimension of x [rows, W]; biased
 * variance from the centred values (two passes over registers), fp32 statistics.  W a multiple of 4, 4 <= W <= 2048.
 * y must not overlap x.
 * SALUN_EINVAL (nothing is written): rows < 1, W outside the domain, eps < 0 or NaN, a NULL pointer, x or y off 16-byte
 * alignment.
 *
 * salun_attn_causal_f32: o = softmax(scale q k^T + causal mask) v per (batch, head), head width D = SALUN_CLIP_ATTN_D,
 * 1 <= T <= SALUN_CLIP_ATTN_MAX_T.  Element (b, t, h, d) of q is qkv[(b T + t) ld + q_off + D h + d], of k and v the
 * same at k_off / v_off (the fused projection buffer [B T, 3 W] has ld = 3 W and offsets 0, W, 2 W); o is written at
 * o[(b T + t) ld_o + D h + d].  Key j > t has weight exactly 0.  o must not overlap qkv.
 * SALUN_EINVAL (nothing is written): D != SALUN_CLIP_ATTN_D, T outside its range, B or H < 1, an offset or a leading
 * dimension that is negative, no multiple of 4 or too small for H D columns, a NULL pointer, qkv or o off 16-byte
 * alignment.
 *
 * salun_quick_gelu: x <- x * sigmoid(1.702 x) in place over n floats (any n; the float4 route needs 16-byte alignment,
 * the scalar route is taken otherwise).
 * SALUN_EINVAL: n < 0, NULL x with n > 0, x off 4-byte alignment. */
#define SALUN_CLIP_ATTN_MAX_T 128
#define SALUN_CLIP_ATTN_D 64
int salun_clip_embed(const int64_t *ids /*dev, B*T*/, const float *tok /*dev, V*W*/, const float *pos /*dev, T*W*/,
                     float *x /*dev, B*T*W*/, int64_t B, int T, int W, int64_t V, salun_stream_t stream);
int salun_ln_f32_forward(const float *x /*dev*/, const float *gamma /*dev, W*/, const float *beta /*dev, W*/,
                         float *y /*dev*/, int64_t rows, int W, double eps, salun_stream_t stream);
int salun_attn_causal_f32(const float *qkv /*dev*/, float *o /*dev*/, int B, int H, int T, int D, int64_t ld, int q_off,
                          int k_off, int v_off, int64_t ld_o, double scale, salun_stream_t stream);
int salun_quick_gelu(float *x /*dev, n*/, int64_t n, salun_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SALUN_H */
