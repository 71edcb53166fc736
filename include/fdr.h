/*
 * fdr.h -- C ABI of libfdr.so: the MI355X (gfx950) frequency-domain restoration path.
 *
 * This is the drop-in boundary for the reference's GPU operator surface.  Every entry point
 * names the reference interface it stands in for (paths relative to the reference repo).
 * Plain pointers and sizes only; no C++ or torch types; every function returns an int status
 * (FDR_OK or a negative FDR_ERR_*), never throws, and leaves a message for fdr_last_error().
 * `stream` arguments are a hipStream_t passed as void* (NULL = the null stream).
 *
 * The C++ shim with the reference's own names (fft_gpu::wienerDeblur_RGB_optimized etc.,
 * fft/fft.hpp:31-45) lives in include/fft/fft.hpp and calls only these functions.
 */
#ifndef FDR_H
#define FDR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FDR_VERSION 300 /* 0.3.0 */

/* status codes (reference: CHECK_CUDA prints and exit(1)s, fft/fft_gpu.cu:59-66; the C++ shim
 * reproduces that on any non-zero status) */
#define FDR_OK 0
#define FDR_ERR_ARG (-1)      /* null pointer, non-positive size, PSF larger than the plan ... */
#define FDR_ERR_NOT_POW2 (-2) /* plan dimensions must be powers of two (callers pad first,
                                 as fft/fft_gpu.cu:287-288 and serial.cpp:36 do) unless
                                 FDR_FLAG_ANY_SIZE asks for the reference's naive-DFT path  */
#define FDR_ERR_HIP (-3)      /* a HIP runtime call failed; message holds hipGetErrorString  */
#define FDR_ERR_STATE (-4)    /* e.g. fdr_wiener_* before fdr_set_psf*                        */
#define FDR_ERR_ALLOC (-5)

/* arithmetic modes of a plan */
#define FDR_MODE_PARITY 0 /* reference operation order (rows, cols, Wiener, rows, cols), per-stage
                             twiddles replayed from the float recurrence of fft/fft_serial.cpp:54-63,
                             no FMA contraction: bit-identical to the serial path's FFT arithmetic */
#define FDR_MODE_FAST 1   /* fused column pass (FFT . Wiener . IFFT), double-generated twiddles (as
                             fft/fft_gpu.cu:206-212), FMA butterflies; within 1e-4 of the serial path */

/* plan flags */
#define FDR_FLAG_SIMPLE_PATH 1u /* reference-shaped kernels: row FFT, transpose, row FFT, transpose
                                   (fft/fft_gpu.cu:214-240); slow, used as an on-device cross-check */

#define FDR_FLAG_FULL_SPECTRUM 32u /* fast mode: keep all N columns of the (Hermitian) spectrum instead of the
                                      non-redundant half (the complex-to-complex byte count of SURVEY.md 8d)     */

#define FDR_FLAG_TABLES_ONLY 1024u /* twiddle tables and min/max scratch only, no M x N workspaces: a plan for the slab
                                      primitives (fdr_slab_*) of the single-image multi-GPU mode, where every rank
                                      holds only its rows of the image; fdr_wiener_* / fdr_fft2d_* / fdr_set_psf*
                                      return FDR_ERR_STATE on such a plan                                          */

#define FDR_FLAG_ANY_SIZE 512u /* accept plan dimensions that are not powers of two: such a dimension is transformed by
                                  the O(n^2) DFT of fft_serial::dft_naive_inplace (fft/fft_serial.cpp:71-87), as
                                  transform_row_inplace dispatches (:100-101) when wienerDeblur_myfft pads to
                                  getOptimalDFTSize (2^a 3^b 5^c, :153-154) instead of to a power of two.  Reference-shaped
                                  passes (rows, transpose, rows, transpose); both modes use the parity arithmetic.        */

#define FDR_FLAG_MIXED_RADIX 2048u /* fast mode: accept plan dimensions 2^a 3^b 5^c up to 8192 -- the sizes getOptimalDFTSize pads to
                                     (fdr_optimal_dft_size, fft/fft_serial.cpp:153-154) -- and transform them by mixed-radix (2/3/4/5)
                                     FFTs on a panel-major full spectrum instead of padding to the next power of two.  Any other size
                                     is refused with FDR_ERR_ARG before device work; FDR_FLAG_ANY_SIZE is not needed and may be set.
                                     With both dimensions powers of two the flag has no effect (the power-of-two path and its limits
                                     hold), so a caller may always pass fdr_optimal_dft_size(rows / cols) with it.  Ignored in parity
                                     mode.  Refused together with FDR_FLAG_TABLES_ONLY or FDR_FLAG_SIMPLE_PATH on such a plan.
                                     fdr_plan_set_batching: `group` images alternate over the workspaces one by one (no multi-image
                                     launches); FDR_OPT_BATCH_GRAPH is accepted and ignored (plain launches) -- as on FDR_FLAG_ANY_SIZE
                                     plans.  fdr_slab_* refuse a non-power-of-two dimension of such a plan.                       */

/* normalisation area selector for fdr_wiener_* */
#define FDR_NORM_PADDED 1  /* serial semantics: min/max over the padded M x N area, then crop
                              (serial.cpp:36-38 + fft/fft_serial.cpp:243-246)                 */
#define FDR_NORM_CROPPED 0 /* reference GPU semantics: min/max over the cropped rows x cols
                              area only (fft/fft_gpu.cu:379-381)                              */
#define FDR_NORM_NONE 2    /* fdr_richardson_lucy_* only: the raw estimate, not normalised (the fdr_wiener_* calls are
                              unchanged: there any value but FDR_NORM_PADDED means CROPPED)  */

typedef struct fdr_plan fdr_plan;

int fdr_version(void);
/* thread-local message of the last failing call on this thread */
const char* fdr_last_error(void);
int fdr_device_count(int* count);

/* -- utils.hpp:27-37,50-52 ------------------------------------------------------------- */
int fdr_next_pow2(int n);
int fdr_is_pow2(int n);

/* -- cv::getOptimalDFTSize as fft/fft_serial.cpp:153-154 uses it: smallest 2^a 3^b 5^c >= n -- */
int fdr_optimal_dft_size(int n);

/* -- plan: owns twiddle tables, the M x N complex workspace, the filter spectrum and the
 *    min/max scratch for one device.  Replaces the per-call cudaMalloc/cudaFree block of
 *    fft/fft_gpu.cu:304-322,389-393.  One host thread at a time per plan.  fdr_plan_destroy
 *    called while the process is already running its exit handlers (static destructors of a
 *    caller) frees the host side only: the HIP runtime may be gone by then.
 *    Dimensions: powers of two up to 32768 (a dimension above 8192 is transformed in 8192-point
 *    blocks plus radix-2 stages in global memory: the reference's serial path takes any power
 *    of two, fft/fft_serial.cpp:90-108); with FDR_FLAG_ANY_SIZE also non-powers of two up to
 *    4096 (naive DFT).  In fast mode with FDR_FLAG_MIXED_RADIX: 2^a 3^b 5^c up to 8192 in each
 *    dimension (mixed-radix FFTs, fast-mode arithmetic); FDR_ERR_ARG otherwise, and the plan
 *    reports FDR_MODE_FAST.                                                               */
int fdr_plan_create(int device, int M, int N, int mode, unsigned flags, fdr_plan** out);
int fdr_plan_destroy(fdr_plan* plan);
int fdr_plan_dims(const fdr_plan* plan, int* M, int* N, int* mode);
/* tunables of a plan */
#define FDR_OPT_TWO_SWEEP_NORM 2   /* fast mode, half spectrum: 1 = the inverse row pass runs twice (min/max only, then
                                      again with the normalisation applied on store) instead of writing a raw real plane
                                      that a normalise pass reads back: 12 instead of 16 bytes per pixel for the last two
                                      passes, same bits (default).  0 = passes C' + E. */
#define FDR_OPT_BATCH_GRAPH 3      /* 1 = fdr_wiener_batch_f32_dev captures its launches (fork, every pass of every group on
                                      the internal streams, join) as a hipGraph on first use and replays it while the call's
                                      arguments stay the same: for small images, whose batches are bound by the host's
                                      launch rate.  0 (default) = plain launches. */
#define FDR_OPT_CE_CHUNK_MB 4      /* batched fast mode on two or more streams: the inverse row passes C1 + C2 of a group of images are
                                      launched in chunks of the group -- as many images as make up at least this many MiB of spectrum
                                      (default 160: pairs at 4096^2, the whole group below) -- because launches of half the size
                                      interleave better with the other stream's memory-bound passes; 0 = always the whole group.
                                      Same bits either way. */
#define FDR_OPT_PAD_MODE 5         /* what the fdr_wiener_* calls put outside the rows x cols picture in the M x N plan:
                                      FDR_PAD_ZERO (default; zeros, as the reference pads) or FDR_PAD_SMOOTH, a smooth periodic
                                      continuation of the picture computed by pass A as it loads (no extra pass, no extra memory).
                                      A photograph is a crop of a larger scene: zero padding gives the periodic blur model a step at
                                      the right and bottom borders and at the wrap to the left and top ones, which the inverse filter
                                      turns into ringing across the whole picture (15 to 19 dB of PSNR).  With
                                      d the picture, e the padded plane and ramp(n)[j] = 0.5 - 0.5 cos(pi (j + 1) / (n + 1)), j < n:
                                          r < rows, c >= cols :  t = ramp(N - cols)[c - cols];  e[r, c] = (1 - t) d[r, cols-1] + t d[r, 0]
                                          r >= rows, all c    :  t = ramp(M - rows)[r - rows];  e[r, c] = (1 - t) e[rows-1, c] + t e[0, c]
                                          result = window( IDFT2( W . DFT2(e) ) ), normalised as with zeros
                                      i.e. to the right of its last column the plane fades into column 0, its wrap neighbour, and below
                                      its last row into row 0.  With rows = M and cols = N there is nothing to fill: same bytes as
                                      FDR_PAD_ZERO.  FDR_NORM_PADDED takes min and max over the whole restored plan (which now holds a
                                      restored continuation), FDR_NORM_CROPPED over the window.  The mode serves fdr_wiener_f32, _dev,
                                      fdr_wiener_batch_f32_dev (part of what an FDR_OPT_BATCH_GRAPH replay is keyed on),
                                      fdr_wiener_batch_f32 and fdr_wiener_batch_ptrs_f32, with a Wiener or a CLS filter.  Leave a margin
                                      of at least the PSF's reach (M >= rows + prows - 1, N >= cols + pcols - 1) for the continuation
                                      to take up the blur that crosses the border.
                                      Not defined: the normalised output of a restored area that is constant.  The flat test that
                                      turns such an area into zeros is exact (max - min below 2.2e-16), a float32 plane that is
                                      constant in exact arithmetic is constant only up to rounding, and (x - min) / (max - min) of
                                      rounding noise is arbitrary in [0, 1].  A constant picture does this on every path and with
                                      either padding; a one-pixel window under FDR_PAD_SMOOTH does it under FDR_NORM_PADDED, because
                                      its continuation is the constant plane (FDR_NORM_CROPPED of one pixel is exactly 0).
                                      Plans: FDR_MODE_FAST on the panel path -- M, N powers of two, 8 .. 8192, with or without
                                      FDR_FLAG_FULL_SPECTRUM.  Parity mode, FDR_FLAG_SIMPLE_PATH, FDR_FLAG_ANY_SIZE sizes, mixed-radix
                                      sizes, FDR_FLAG_TABLES_ONLY and dimensions below 8 or above 8192 return FDR_ERR_ARG before any
                                      device work, as does any other value.  The blur operator, Richardson-Lucy (both forms), the TV
                                      solve, the motion estimate, fdr_batch_run (its own plans) and fdr_slab_* pad with zeros and
                                      ignore the option. */
#define FDR_PAD_ZERO 0
#define FDR_PAD_SMOOTH 1
int fdr_plan_set_option(fdr_plan* plan, int option, long long value);

/* -- PSF generation: utils.hpp:15-24 motionBlurKernel(size, angle) ------------------- */
/* host result, size*size floats (computed on the device by the psf kernel, copied back) */
int fdr_psf_motion(int size, double angle_deg, float* out_host);
/* device result into d_out (size*size floats), asynchronous on stream */
int fdr_psf_motion_dev(int device, int size, double angle_deg, float* d_out, void* stream);

/* -- the OpenCV call inside motionBlurKernel (utils.hpp:22): cv::warpAffine(src, dst, M, dsize) with its defaults
 *    (INTER_LINEAR, BORDER_CONSTANT 0) on a single-channel float image, evaluated on the device in OpenCV's classic
 *    fixed-point form (10-bit coordinates rounded to 1/32 pixel, 32 x 32 float weight table).
 *    M: the 2 x 3 forward matrix (row-major) as cv::getRotationMatrix2D returns it; inverted in double as
 *    cv::warpAffine does.  Host pointers; strides in elements.  fdr_psf_motion(size, angle) is this call applied to
 *    the line kernel of utils.hpp:17-19 with the matrix of :20 (same bits).                                          */
int fdr_warp_affine_f32(const float* src_host, int srows, int scols, int sstride, const double M[6],
                        float* dst_host, int drows, int dcols, int dstride);

/* -- PSF spectrum: pad top-left + forward 2-D FFT (fft/fft_serial.cpp:166-171,182;
 *    fft/fft_gpu.cu:340,356), kept in the plan together with K.                        */
int fdr_set_psf(fdr_plan* plan, const float* psf_host, int prows, int pcols, int pstride, float K);
int fdr_set_psf_dev(fdr_plan* plan, const float* d_psf, int prows, int pcols, int pstride, float K, void* stream);
/* motionBlurKernel on the device straight into the plan (no host round trip) */
int fdr_set_psf_motion(fdr_plan* plan, int size, double angle_deg, float K, void* stream);

/* -- constrained least-squares (CLS) filter (Gonzalez & Woods 5.9), the second filter the reference's prototype names
 *    (others/fft_image_restoration.py:109-112, constrained_least_square_filtering, never defined there).  The same three calls
 *    with a smoothness weight gamma: for bin (u, v) of the M x N plan
 *        W = conj(H) / (|H|^2 + K + gamma L^2),   L = 4 sin^2(pi u / M) + 4 sin^2(pi v / N)
 *    L is the symbol of the periodic 5-point Laplacian [[0,-1,0],[-1,4,-1],[0,-1,0]], so roughness is penalised instead of
 *    energy.  Evaluated in double, rounded once; a zero denominator gives W = 0.  The filter then serves every fdr_wiener_*
 *    call (batches, FDR_OPT_BATCH_GRAPH replays) and travels with fdr_plan_export_filter_dev / fdr_plan_import_filter_dev.
 *    Validation, plan state and the PRE phase as the fdr_set_psf* counterparts; the first call on a plan also uploads a table
 *    of M + N doubles (kept until fdr_plan_destroy).
 *      gamma == 0          exactly the Wiener call (same filter bytes)
 *      gamma < 0, NaN, inf FDR_ERR_ARG before any device work
 *      gamma > 0           FDR_MODE_FAST plans only: a parity-mode plan (so every FDR_FLAG_ANY_SIZE plan with a non-power-of-two
 *                          dimension) returns FDR_ERR_ARG before any device work, its previous filter intact -- parity mode is
 *                          bit-identical to ./serial, which has no CLS
 *      tables-only plans   FDR_ERR_STATE
 *    fdr_slab_* and fdr_batch_run have the Wiener filter only.                                                         */
int fdr_set_psf_cls(fdr_plan* plan, const float* psf_host, int prows, int pcols, int pstride, float K, float gamma);
int fdr_set_psf_cls_dev(fdr_plan* plan, const float* d_psf, int prows, int pcols, int pstride, float K, float gamma, void* stream);
int fdr_set_psf_motion_cls(fdr_plan* plan, int size, double angle_deg, float K, float gamma, void* stream);

/* -- the prepared filter of a plan as an opaque block of bytes, for a caller that distributes ONE rank's PSF spectrum to the
 *    others instead of recomputing it everywhere -- the role of the MPI_Bcast / MPI_Scatterv of the padded PSF in the
 *    reference's MPI variant (fft/fft_mpi.cpp:334-378); in the batched mode a broadcast over RCCL (bench.py --bcast-filter).
 *    The layout is private to the library (mode, flags and dimensions select it): a block exported from one plan may only be
 *    imported into a plan created with the same (M, N, mode, flags) -- on any device.  `bytes` is the exact size.
 *      fdr_plan_filter_bytes   size of the block (FDR_ERR_STATE on a tables-only plan)
 *      fdr_plan_export_filter_dev  copy the plan's filter into d_dst (device memory of the plan's device), asynchronous on stream;
 *                                  needs a PSF set on the plan
 *      fdr_plan_import_filter_dev  copy d_src in as the plan's filter and take K with it: the plan then behaves as after
 *                                  fdr_set_psf* with the exporting plan's PSF                                              */
int fdr_plan_filter_bytes(const fdr_plan* plan, size_t* bytes);
int fdr_plan_export_filter_dev(fdr_plan* plan, void* d_dst, size_t bytes, void* stream);
int fdr_plan_import_filter_dev(fdr_plan* plan, const void* d_src, size_t bytes, float K, void* stream);

/* -- the operator: fft_serial::wienerDeblur_myfft (fft/fft_serial.cpp:141-261) wrapped as
 *    serial.cpp:34-39 does (pad -> restore -> crop), one channel.  img rows x cols with row
 *    stride `stride` (elements); out rows x cols with row stride `out_stride`, values in [0,1].
 *    rows <= M, cols <= N.  Host-pointer form copies in and out synchronously; the _dev form
 *    is asynchronous on `stream` and touches only device memory.                         */
int fdr_wiener_f32(fdr_plan* plan, const float* img_host, int rows, int cols, int stride,
                   float* out_host, int out_stride, int norm_area);
int fdr_wiener_f32_dev(fdr_plan* plan, const float* d_img, int rows, int cols, int stride,
                       float* d_out, int out_stride, int norm_area, void* stream);
/* `count` independent images, image i at d_imgs + i*img_pitch / d_out + i*out_pitch (elements);
 * the batched mode of BASELINE config 5 (one plan, one PSF spectrum, many images).      */
int fdr_wiener_batch_f32_dev(fdr_plan* plan, const float* d_imgs, size_t img_pitch, int count,
                             int rows, int cols, int stride,
                             float* d_out, size_t out_pitch, int out_stride, int norm_area, void* stream);

/* -- the forward blur operator and Richardson-Lucy deconvolution (RL; Richardson 1972, Lucy 1974: the iterative maximum-likelihood
 *    deconvolution for Poisson noise, MATLAB's deconvlucy / scikit-image's richardson_lucy).  The plan is M x N, the image window
 *    rows x cols at its top-left corner; pad(x) is x on the window and 0 elsewhere; the operator PSF p lies top-left in an M x N
 *    zero plane exactly as fdr_set_psf places it, and H = DFT2(p), so RL and the Wiener filter invert the same blur model:
 *        blur(x)   = window( IDFT2( H       . DFT2(pad(x)) ) )      (IDFT2 includes 1/(M N): a delta PSF gives blur(x) = x)
 *        blur^T(y) = window( IDFT2( conj(H) . DFT2(pad(y)) ) )      (the adjoint: <blur x, y> = <x, blur^T y>)
 *    Circular convolution on the plan: with rows = M, cols = N and a PSF the caller has rolled to put its centre at (0, 0),
 *    fft_convolve of the reference's others/gen_blurred_img.ipynb.  RL with n iterations on the input window d:
 *        d+ = max(d, 0);  u = d+;  n times:  c = blur(u);  r = c > FDR_RL_TAU ? d+ / c : 0;  u = max(u . blur^T(r), 0)
 *    and the output is u on the window, normalised by norm_area: FDR_NORM_NONE the raw estimate, FDR_NORM_CROPPED min-max to
 *    [0, 1] over the window, FDR_NORM_PADDED min-max over the M x N plan (u is 0 outside the window); a flat result comes out as
 *    the fdr_wiener_* calls give a flat plane (all 0).  n = 0 returns d+.  Outside the window u and r stay 0.
 *    Plans: FDR_MODE_FAST, M and N powers of two, 8 <= M <= 8192, 32 <= N <= 8192, neither FDR_FLAG_SIMPLE_PATH nor
 *    FDR_FLAG_FULL_SPECTRUM (FDR_FLAG_MIXED_RADIX has no effect on such sizes); every other plan returns FDR_ERR_ARG before any
 *    device work, a tables-only plan FDR_ERR_STATE, and the plan stays usable.  fdr_wiener_batch_*, fdr_batch_run, fdr_slab_* and
 *    filter export / import do not cover the operator; several images per launch are fdr_blur_batch_f32_dev and
 *    fdr_richardson_lucy_batch_f32* below.
 *      fdr_set_operator_psf*   the operator PSF (validated as in fdr_set_psf*), held apart from the Wiener / CLS filter: setting
 *                              either never changes the other.  The first call on a plan allocates the two operator tables
 *                              (2 x fdr_plan_filter_bytes), kept until fdr_plan_destroy.  PRE phase.
 *      fdr_blur_f32*           out = blur(img), or blur^T(img) with adjoint != 0.  FDR_ERR_STATE without an operator PSF.
 *      fdr_richardson_lucy_f32*  n = iterations >= 0; FDR_ERR_ARG for a negative count, an unknown norm_area or an output
 *                              window that overlaps the input (d is read on every iteration, u is kept in the output).
 *    Shape errors as fdr_wiener_*.  The _dev forms are asynchronous on `stream` and allocate nothing; the host forms copy in
 *    and out synchronously and count as COMPUTE (as fdr_wiener_f32).  A 4096^2 iteration moves about 64 bytes per padded
 *    pixel.                                                                                        */
#define FDR_RL_TAU 1e-7f /* the guard of the RL ratio: a blurred estimate c <= FDR_RL_TAU gives r = 0 */
int fdr_set_operator_psf(fdr_plan* plan, const float* psf_host, int prows, int pcols, int pstride);
int fdr_set_operator_psf_dev(fdr_plan* plan, const float* d_psf, int prows, int pcols, int pstride, void* stream);
int fdr_set_operator_psf_motion(fdr_plan* plan, int size, double angle_deg, void* stream);
int fdr_blur_f32(fdr_plan* plan, const float* img_host, int rows, int cols, int stride, float* out_host, int out_stride, int adjoint);
int fdr_blur_f32_dev(fdr_plan* plan, const float* d_img, int rows, int cols, int stride, float* d_out, int out_stride, int adjoint,
                     void* stream);
int fdr_richardson_lucy_f32(fdr_plan* plan, const float* img_host, int rows, int cols, int stride, float* out_host, int out_stride,
                            int iterations, int norm_area);
int fdr_richardson_lucy_f32_dev(fdr_plan* plan, const float* d_img, int rows, int cols, int stride, float* d_out, int out_stride,
                                int iterations, int norm_area, void* stream);

/* -- free-boundary, weighted Richardson-Lucy (Bertero & Boccacci 2005, "A simple method for the reduction of boundary effects in the
 *    Richardson-Lucy approach to image deconvolution"; the WEIGHT argument of MATLAB's deconvlucy): RL for a picture that is a crop
 *    of a larger scene.  The calls above take the plan for periodic (or the window for surrounded by zeros), so the light that the
 *    blur carried in from outside the frame is taken for signal and the error grows inward with every iteration.  Here the estimate u
 *    lives on the whole M x N plan, the data d (rows x cols at the top-left corner) constrain it inside the window only, and per-pixel
 *    weights m in [0, 1] (rows x cols, row stride wstride; NULL = all ones; 0 = ignore this pixel: dead, saturated, cosmic ray)
 *    say how much each datum counts.  H is the operator spectrum of fdr_set_operator_psf*, pad(x) is x on the window and 0 elsewhere:
 *        fullblur(x) = IDFT2( H . DFT2(x) ),  fullblur^T(y) = IDFT2( conj(H) . DFT2(y) )      (whole plan; IDFT2 includes 1/(M N))
 *        W = pad(m);  dw = pad(m . max(d, 0))
 *        alpha = fullblur^T(W)                                 (the coverage: how much data sees each plan pixel)
 *        wgt = alpha > sigma ? 1 / alpha : 0
 *        u   = alpha > sigma ? sum(dw) / sum(W) : 0            (both sums in double, in a fixed order; 0 when sum(W) = 0)
 *        n times:  c = window(fullblur(u));  r = c > FDR_RL_TAU ? dw / c : 0  (0 outside the window);  u = max(u . wgt . fullblur^T(pad(r)), 0)
 *    The output is the top-left out_rows x out_cols of u, rows <= out_rows <= M, cols <= out_cols <= N (with M x N the caller gets
 *    the extrapolated surround too), normalised over that output window by norm_area exactly as fdr_richardson_lucy_* defines
 *    FDR_NORM_NONE / _CROPPED / _PADDED (PADDED counts one 0 when the output window is smaller than the plan).  n = 0 returns the
 *    start.  sigma in (0, 1) cuts plan pixels that almost no datum sees (FDR_RL_SIGMA is the usual choice).  Wherever c > tau,
 *    sum(alpha . u) = sum(dw) after every iteration: the free-boundary form of flux conservation.
 *    With M >= rows + prows - 1 and N >= cols + pcols - 1 the two far borders of the window do not couple through the wrap of the
 *    plan; this is not enforced: a full-plane window is legal, and then alpha = sum(psf) everywhere and an iteration is a plain RL
 *    step.  A PSF placed top-left works without the c = 0 border rows of the calls above (u is non-zero outside the window); the
 *    result is then shifted by the PSF's half-size, as for the Wiener calls.  Weights outside [0, 1] are not checked.
 *    Plans and refusals as fdr_richardson_lucy_f32* (FDR_ERR_STATE without an operator PSF), and FDR_ERR_ARG for a null params
 *    pointer, sigma outside (0, 1), a weights stride below cols, an output window outside [rows .. M] x [cols .. N] or with
 *    out_stride < out_cols, or an output that overlaps the input or the weights; always before any device work, the plan usable
 *    afterwards.  The first call on a plan allocates the workspace, kept until fdr_plan_destroy: three M x N float planes (u, wgt,
 *    dw) and the partials of the two sums, 12 M N bytes; FDR_ERR_ALLOC, plan intact, if it cannot be had.  After it the _dev form
 *    allocates nothing and is asynchronous on `stream`; the coverage is recomputed by every call (one adjoint blur: the weights may
 *    have changed).  The host form copies in and out synchronously and counts as COMPUTE.  The Wiener / CLS filter, the operator
 *    tables, the TV and motion workspaces and the results of every other call stay as they were.  An iteration moves about 68
 *    bytes per plan pixel with a full-plane window.                                                    */
#define FDR_RL_SIGMA 1e-2f /* the usual coverage threshold of the free-boundary calls */
typedef struct fdr_rlfree_params {
    int iterations; /* >= 0 */
    float sigma;    /* coverage threshold, in (0, 1) */
    int norm_area;  /* FDR_NORM_NONE / FDR_NORM_CROPPED / FDR_NORM_PADDED, over the output window */
    int out_rows;   /* rows .. M */
    int out_cols;   /* cols .. N */
} fdr_rlfree_params;
int fdr_richardson_lucy_free_f32(fdr_plan* plan, const float* img_host, int rows, int cols, int stride, const float* weights_host,
                                 int wstride, float* out_host, int out_stride, const fdr_rlfree_params* params);
int fdr_richardson_lucy_free_f32_dev(fdr_plan* plan, const float* d_img, int rows, int cols, int stride, const float* d_weights,
                                     int wstride, float* d_out, int out_stride, const fdr_rlfree_params* params, void* stream);

/* -- batched blur and Richardson-Lucy: `count` images with one operator PSF, several per launch.  Image i is read at d_imgs + i img_pitch
 *    and written at d_out + i out_pitch (elements), as in fdr_wiener_batch_f32_dev; a colour picture is three such planes.  The call
 *    cuts the batch into launch groups of `group` images (fdr_plan_set_batching; the last group may be smaller) and every pass of a
 *    group -- the forward rows, the column pass, the inverse rows with the ratio or the update -- is ONE launch over its images, so
 *    the operator table is read once per group and a small image no longer leaves the chip idle.  A group runs to completion (start,
 *    every iteration, normalisation) on the caller's stream, on the workspaces 0 .. group - 1 that fdr_plan_set_batching made, before
 *    the next begins; nstreams above 1 and FDR_OPT_BATCH_GRAPH are accepted and change nothing here, and group = 1 (the default) is
 *    literally the loop of the single-image _dev calls.  The maths is that of the single-image calls and so are the bits: every image
 *    of a batch comes out bit for bit as the single-image _dev call of the same form gives it on the same plan, for every group size,
 *    tail and layout.
 *      fdr_blur_batch_f32_dev             fdr_blur_f32_dev per image.
 *      fdr_richardson_lucy_batch_f32_dev  params->free_boundary == 0: fdr_richardson_lucy_f32_dev per image (u in each output window,
 *                              r in each workspace: no allocation); out_rows = out_cols = 0 or rows, cols; weights must be NULL.
 *                              free_boundary != 0: fdr_richardson_lucy_free_f32_dev per image with ONE weights plane (rows x cols, row
 *                              stride wstride; NULL = all ones) for the whole batch: the setup of image 0, the coverage alpha and wgt
 *                              are computed once per call, every image has its own dw, its own sums and its own M x N estimate, and
 *                              the output window is out_rows x out_cols per image.  The first such call with a group g > 1 grows the
 *                              free-boundary workspace from three to 1 + 2 g planes (4 (1 + 2 g) M N bytes and g sets of partials);
 *                              FDR_ERR_ALLOC leaves the plan and the three-plane workspace as they were.  (The start of images after
 *                              the first thresholds wgt > 0 in place of alpha > sigma: the same for every finite alpha.)
 *      fdr_richardson_lucy_batch_f32      host pointers, synchronous: every image in, the batch, every result back.
 *    Refusals, always before any device work and with the plan usable afterwards: a negative count (count = 0 returns FDR_OK at
 *    once), a null pointer, whatever the single-image call of the form refuses for one image (plan, operator PSF, window, strides,
 *    iterations, norm_area, sigma, the output window), weights in the plain form, and an output that overlaps the input or the
 *    weights anywhere within the span of the batch (first element of image 0 to last element of image count - 1).  Neither _dev
 *    form allocates after its first call, and both stay asynchronous on `stream`.  The accelerated iteration has the batched form
 *    fdr_richardson_lucy_batch_accel_f32* below and TV the batched form fdr_tv_deconv_batch_f32*; the data-stopped and blind
 *    iterations, per-image weights, mixed-radix and full-spectrum plans and fdr_batch_run have none (DESIGN.md sections 24, 29 and 30).
 *    Per image and iteration a group of g moves 64 - 8 (1 - 1/g) bytes per padded pixel.                                        */
int fdr_blur_batch_f32_dev(fdr_plan* plan, const float* d_imgs, size_t img_pitch, int count, int rows, int cols, int stride,
                           float* d_out, size_t out_pitch, int out_stride, int adjoint, void* stream);
typedef struct fdr_rl_batch_params {
    int iterations;     /* >= 0 */
    int norm_area;      /* FDR_NORM_NONE / _CROPPED / _PADDED, per image */
    int free_boundary;  /* 0: fdr_richardson_lucy_f32's iteration; 1: fdr_richardson_lucy_free_f32's */
    float sigma;        /* free form: coverage threshold in (0, 1) */
    int out_rows, out_cols; /* free form: rows..M, cols..N; plain form: rows, cols (0, 0 means the same) */
} fdr_rl_batch_params;
int fdr_richardson_lucy_batch_f32_dev(fdr_plan* plan, const float* d_imgs, size_t img_pitch, int count, int rows, int cols, int stride,
                                      const float* d_weights, int wstride, float* d_out, size_t out_pitch, int out_stride,
                                      const fdr_rl_batch_params* params, void* stream);
int fdr_richardson_lucy_batch_f32(fdr_plan* plan, const float* imgs_host, size_t img_pitch, int count, int rows, int cols, int stride,
                                  const float* weights_host, int wstride, float* out_host, size_t out_pitch, int out_stride,
                                  const fdr_rl_batch_params* params);

/* -- accelerated Richardson-Lucy: Biggs & Andrews' vector extrapolation ("Acceleration of iterative image restoration algorithms",
 *    Applied Optics 36, 1997; the default of MATLAB's deconvlucy) around the unchanged iteration of either form above.  With
 *    step(y) one iteration applied to y (plain form: c = blur(y), r = c > FDR_RL_TAU ? d+ / c : 0, step(y) = max(y . blur^T(r), 0) on
 *    the window; free-boundary form: c = window(fullblur(y)), r likewise from dw, step(y) = max(y . wgt . fullblur^T(pad(r)), 0) on the
 *    whole plan, with setup, coverage, wgt and the start exactly as above) and u_0 the start of the plain call:
 *        k = 0, 1 :  alpha_k = 0;  y_k = u_k
 *        k >= 2   :  alpha_k = clamp( sum(g_(k-1) . g_(k-2)) / sum(g_(k-2) . g_(k-2)), 0, FDR_RL_ACCEL_MAX )
 *                    (0 when the denominator is 0 or the quotient is not finite)
 *                    y_k = max(u_k + alpha_k (u_k - u_(k-1)), 0)
 *        every k  :  u_(k+1) = step(y_k);   g_k = u_(k+1) - y_k
 *    The output is u_n, normalised or cropped exactly as the plain calls do it.  The sums run over the window (plain form) or the
 *    whole M x N plan (free-boundary form), in double and in a fixed order (per-workgroup partials, then one workgroup; no float
 *    atomics), so results are bit-identical from call to call; alpha is rounded to float once and stays on the device: the _dev
 *    forms make no host read-back and stay asynchronous on `stream`.  alpha_0 = alpha_1 = 0, so n <= 2 gives the bits of the plain
 *    calls (and launches nothing else).  Every u_k is the output of a step, so the flux identities of the plain calls hold.  Per
 *    iteration the extrapolation adds one inner-product pass and one pointwise pass, about 28 bytes per pixel of the estimate, and
 *    no transform; it typically reaches in 10 iterations what the plain calls need 20 to 30 for, and fits noise sooner as well
 *    (DESIGN.md section 21).
 *    alphas may be NULL; otherwise it receives `iterations` floats, alpha_0 .. alpha_(n-1).  Plans, refusals, overlap rules, phases
 *    and norm_area as the plain counterparts; the _dev forms also return FDR_ERR_ARG for a d_alphas range that overlaps the output,
 *    the input or the weights.  The first accelerated call on a plan (either form) allocates the workspace both forms share, kept
 *    until fdr_plan_destroy: three M x N float planes (y, the second plane of the estimate, g), the double partials and alpha,
 *    12 M N + 16 ceil(M / 8) ceil(N / 1024) + 8 bytes; FDR_ERR_ALLOC, plan intact, if it cannot be had.  After it the _dev forms
 *    allocate nothing (the free-boundary form needs its own workspace as before).  The plain form's estimate alternates between
 *    d_out and the workspace; the input is still read on every iteration.                                                       */
#define FDR_RL_ACCEL_MAX 0.9990234375f /* 1 - 2^-10: the upper bound of the extrapolation factor */
int fdr_richardson_lucy_accel_f32(fdr_plan* plan, const float* img_host, int rows, int cols, int stride, float* out_host, int out_stride,
                                  int iterations, int norm_area, float* alphas_host);
int fdr_richardson_lucy_accel_f32_dev(fdr_plan* plan, const float* d_img, int rows, int cols, int stride, float* d_out, int out_stride,
                                      int iterations, int norm_area, float* d_alphas, void* stream);
int fdr_richardson_lucy_free_accel_f32(fdr_plan* plan, const float* img_host, int rows, int cols, int stride, const float* weights_host,
                                       int wstride, float* out_host, int out_stride, const fdr_rlfree_params* params, float* alphas_host);
int fdr_richardson_lucy_free_accel_f32_dev(fdr_plan* plan, const float* d_img, int rows, int cols, int stride, const float* d_weights,
                                           int wstride, float* d_out, int out_stride, const fdr_rlfree_params* params, float* d_alphas,
                                           void* stream);

/* -- batched accelerated Richardson-Lucy: fdr_richardson_lucy_batch_f32* with the accelerated iteration above, several images per
 *    launch.  Arguments, launch groups, forms, workspaces and refusals are those of fdr_richardson_lucy_batch_f32*, and params is the
 *    same struct.  Per iteration a group makes the launches of one image: one extrapolation, one direction and one alpha launch over
 *    the group (the image is the third grid dimension), every image with its own inner products, its own partials and its own alpha,
 *    folded in the single-image order.  Every image and every alpha comes out bit for bit as fdr_richardson_lucy_accel_f32_dev or
 *    fdr_richardson_lucy_free_accel_f32_dev gives it for that image alone on the same plan, for every group size, tail and layout;
 *    iterations <= 2 gives the bits of fdr_richardson_lucy_batch_f32*.  group = 1 is literally the loop of the single accelerated
 *    calls.  d_alphas may be NULL; otherwise image i receives `iterations` floats at d_alphas + i alpha_pitch (elements), and
 *    alpha_pitch >= iterations is required.  Refused as well, before any device work: alpha_pitch < iterations with alphas given,
 *    and an alphas range (first float of image 0 to last float of image count - 1) that overlaps the inputs, the outputs or the
 *    weights of the batch.  The first call with a group g > 1 grows the acceleration workspace to g images (g (12 M N + 16 ceil(M / 8)
 *    ceil(N / 1024)) + 32 bytes; the new block is had before the old one is freed, FDR_ERR_ALLOC leaves the plan and the old
 *    workspace usable); after it the _dev form allocates nothing and stays asynchronous on `stream`, with no host read-back.  Per
 *    image and iteration the extrapolation adds its 28 bytes per pixel of the estimate, which a group does not share (DESIGN.md
 *    section 29).  The host form stages as fdr_richardson_lucy_batch_f32 and is synchronous.                                    */
int fdr_richardson_lucy_batch_accel_f32_dev(fdr_plan* plan, const float* d_imgs, size_t img_pitch, int count, int rows, int cols, int stride,
                                            const float* d_weights, int wstride, float* d_out, size_t out_pitch, int out_stride,
                                            const fdr_rl_batch_params* params, float* d_alphas, size_t alpha_pitch, void* stream);
int fdr_richardson_lucy_batch_accel_f32(fdr_plan* plan, const float* imgs_host, size_t img_pitch, int count, int rows, int cols, int stride,
                                        const float* weights_host, int wstride, float* out_host, size_t out_pitch, int out_stride,
                                        const fdr_rl_batch_params* params, float* alphas_host, size_t alpha_pitch);

/* -- Richardson-Lucy that stops from the data: the fit trace and the discrepancy rules.  The iteration count is RL's only
 *    regularisation: on noisy data the estimate first sharpens, then fits the noise.  These calls run any of the four forms above
 *    (free_boundary, accelerate) and measure, inside the ratio pass of every step and at no extra pass, how well the reblurred
 *    point fits the data.  With c = blur(y_k) on the window (y_k = u_k in the plain forms, the extrapolated point in the
 *    accelerated ones: the input of step k), d+ = max(d, 0) and w the pixel's weight (1 in the plain form; m, or 1 for NULL weights,
 *    in the free-boundary form):
 *        res_k = sum w (d+ - c)^2
 *        kl_k  = sum w ( c - d+ + (d+ > 0 && c > FDR_RL_TAU ? d+ ln(d+ / c) : 0) )          (the generalised Kullback-Leibler distance)
 *    both over the window, in double and in a fixed order (each thread adds its terms in order, a fixed tree per workgroup, one
 *    workgroup folds the partials in index order; no atomics), so a trace is bit-identical from call to call.  trace[2 k] = res_k,
 *    trace[2 k + 1] = kl_k.  With S = rows cols (plain form) or S = sum(W), the double sum of the setup (free-boundary form):
 *        FDR_RL_STOP_NONE      `iterations` steps, the trace only.
 *        FDR_RL_STOP_RESIDUAL  Gaussian noise (Morozov's discrepancy principle): stat_k = res_k, target = tau sigma^2 S; sigma = 0
 *                              estimates it from the window (fdr_noise_sigma; the weights are not looked at).
 *        FDR_RL_STOP_KL        Poisson noise, d in units of 1 / gain photons (Bertero, Boccacci, Talenti, Zanella, Zanni 2010, "A
 *                              discrepancy principle for Poisson data"): stat_k = 2 gain kl_k / S, target = tau.
 *    k* is the first k with stat_k <= target.  The step in flight is always finished and the host looks only after every
 *    check_every steps: iterations_done = min(n, c ceil((k* + 1) / c)), c = check_every; without such a k, iterations_done = n and
 *    stopped = 0.  The output is u_(iterations_done): bit for bit what the call of the same form returns for iterations =
 *    iterations_done with the same norm_area and output window.  result->sigma is the sigma used (RESIDUAL; else the one passed),
 *    result->target the target, result->statistic the last stat_k the decision looked at (stat_k* when it stopped, else that of
 *    the last step); target and statistic are 0 with FDR_RL_STOP_NONE.  trace may be NULL; otherwise it receives
 *    2 iterations_done doubles (room for 2 n is needed).
 *    With FDR_RL_STOP_NONE the _dev form makes no read-back, stays asynchronous on `stream` and allocates nothing after the first
 *    call.  With a rule it is synchronous, as fdr_choose_reg_f32_dev is: it reads 2 check_every doubles back every check_every
 *    steps (and sum(W), and the noise sum for sigma = 0, once).  The rule errs on the early side: it stops at the first iterate
 *    that fits to within the noise, which on the scenes tried lay at or up to 0.2 dB below the best iterate and always above the
 *    blurred input; in the accelerated forms the trace speaks of y_k, not of u_k; a textured picture
 *    inflates the estimated sigma and so stops earlier still.
 *    Plans, refusals, overlap rules and phases are those of the underlying form (cov_sigma, out_rows and out_cols are the sigma,
 *    out_rows and out_cols of fdr_rlfree_params; the plain form takes out_rows = out_cols = 0 or rows, cols).  FDR_ERR_ARG also for
 *    a null params or result, an unknown rule, KL with a gain that is not finite and > 0, a sigma or tau that is negative or not
 *    finite, check_every < 0, a weights pointer in the plain form, a window below 3 x 3 when sigma is to be estimated, and a
 *    d_trace range (2 n doubles) that overlaps a window; always before any device work, the plan usable afterwards.  The first
 *    call on a plan allocates the workspace, kept until fdr_plan_destroy: 16 bytes per workgroup of the inverse row pass, the
 *    partials of the noise estimate, an internal trace of 1024 steps (it grows only for a call with a rule, without the caller's
 *    trace and with more steps than that) and, for the free-boundary form with weights, two M x N float planes (the dense weights
 *    and the dense copy of d: the ratio pass forms dw = w d+ itself, the float product of the setup); FDR_ERR_ALLOC, plan intact, if
 *    it cannot be had.  The workspaces of the underlying form are needed as before.                                                      */
#define FDR_RL_STOP_NONE 0     /* run `iterations` steps, record the trace only */
#define FDR_RL_STOP_RESIDUAL 1 /* Gaussian noise: res_k <= tau sigma^2 S */
#define FDR_RL_STOP_KL 2       /* Poisson noise (Bertero et al. 2010): 2 gain kl_k / S <= tau */
typedef struct fdr_rl_auto_params {
    int iterations;    /* the most steps taken, >= 0 */
    int free_boundary; /* 0: the plain form; else the free-boundary, weighted form */
    int accelerate;    /* 0: the plain iteration; else Biggs & Andrews' extrapolation */
    int rule;          /* FDR_RL_STOP_* */
    float sigma;       /* RESIDUAL: noise standard deviation; 0 = fdr_noise_sigma of the window */
    float gain;        /* KL: photons per unit of d, > 0 */
    float tau;         /* 0 = 1 */
    int check_every;   /* 0 = 1 */
    int norm_area;     /* FDR_NORM_NONE / FDR_NORM_CROPPED / FDR_NORM_PADDED */
    float cov_sigma;   /* free form: as fdr_rlfree_params.sigma */
    int out_rows;      /* free form: as fdr_rlfree_params; plain form: 0 or rows */
    int out_cols;      /* free form: as fdr_rlfree_params; plain form: 0 or cols */
} fdr_rl_auto_params;
typedef struct fdr_rl_auto_result {
    int iterations_done;
    int stopped; /* 1: the rule fired; 0: `iterations` steps were taken */
    double sigma, target, statistic;
} fdr_rl_auto_result;
int fdr_richardson_lucy_auto_f32(fdr_plan* plan, const float* img_host, int rows, int cols, int stride, const float* weights_host,
                                 int wstride, float* out_host, int out_stride, const fdr_rl_auto_params* params,
                                 fdr_rl_auto_result* result, double* trace_host);
int fdr_richardson_lucy_auto_f32_dev(fdr_plan* plan, const float* d_img, int rows, int cols, int stride, const float* d_weights,
                                     int wstride, float* d_out, int out_stride, const fdr_rl_auto_params* params,
                                     fdr_rl_auto_result* result, double* d_trace, void* stream);

/* -- blind Richardson-Lucy (Fish, Brinicombe, Pike & Walker 1995, "Blind deconvolution by means of the Richardson-Lucy algorithm";
 *    Holmes 1992; MATLAB's deconvblind): the PSF takes the same multiplicative maximum-likelihood step as the image, from the same
 *    ratio.  The call REFINES a PSF: it does not find one from nothing.  A flat start does not move (the symmetric saddle), a zero
 *    of the start stays zero for good (that is how a caller masks the support), and the PSF is determined only up to a shift inside
 *    its support, with the image shifted the other way.  The usual start is fdr_psf_gaussian.
 *    The plan is M x N, the window rows x cols at its top-left corner, p_k the prows x pcols PSF top-left in the plan as
 *    fdr_set_operator_psf places it, H_k = DFT2(pad(p_k)), and
 *        corr_u(y) = IDFT2( conj(DFT2(u)) . DFT2(y) ), cropped to the top-left prows x pcols
 *    Plain form (blur, d+ and u_0 = d+ as in fdr_richardson_lucy_f32, blur_k with p_k):
 *        every k:        c = blur_k(u_k);  r = c > FDR_RL_TAU ? d+ / c : 0
 *                        u_(k+1) = max(u_k . blur_k^T(r), 0)                          (exactly the step of fdr_richardson_lucy_f32 with p_k)
 *        k >= psf_hold:  q = max(p_k . corr_(u_k)(pad(r)), 0);  s = sum(q)            (s in double, in a fixed order)
 *                        p_(k+1) = s > 0 and finite ? q / s : p_k
 *        k <  psf_hold:  p_(k+1) = p_k
 *    Both updates use the same r and the iterates of step k (the joint, Jacobi form).
 *    Free-boundary, weighted form (W, dw, fullblur and sigma as in fdr_richardson_lucy_free_f32): the coverage alpha_k =
 *    fullblur_k^T(W) and wgt_k are recomputed from every new p_k, u_0 is that form's start under p_0, the image step is that form's
 *    step with p_k, and the PSF step is the exact EM step
 *        num = corr_(u_k)(pad(r));  den = corr_(u_k)(W);  q = den > 0 ? max(p_k . num / den, 0) : 0;  then s and p_(k+1) as above
 *    So p_k >= 0 and sum(p_k) = 1 for every k >= 1 that followed an update, psf_hold >= iterations is the non-blind call (the bits of
 *    fdr_richardson_lucy_f32 / _free_f32 with p_0, the PSF untouched), and a 1 x 1 PSF stays {1}.  On a CROPPED window use the
 *    free-boundary form: the plain form's periodic model is wrong at the rim and its PSF does not converge there.
 *    Output: u_n on the output window, normalised as in the underlying form, and p_n in place of the start PSF.  On return the
 *    plan's operator tables are those of p_n (every PSF update rebuilds them, as fdr_set_operator_psf_dev does): fdr_blur_*, the RL
 *    calls, fdr_tv_deconv_* and fdr_choose_reg_* follow directly.  An operator PSF need not have been set before.
 *    Plans, refusals, overlap rules and phases are those of the underlying form.  FDR_ERR_ARG, before any device work and with the
 *    plan usable afterwards, also for: a null params or PSF pointer, psf_hold < 0, a PSF that is empty, larger than the plan or of
 *    more than FDR_BLIND_MAX_PSF entries, pstride < pcols, weights in the plain form, a plain-form output window other than 0, 0 or
 *    rows, cols, a PSF range that overlaps the input, the weights or the output, a free-boundary window smaller than the PSF (the
 *    minimum is prows x pcols: under a smaller one the shifted window of a tap's den can lie wholly where the coverage is below
 *    sigma, u = 0 there, and the sign of den -- the tap itself -- would be rounding noise), and -- host form -- a start PSF with a negative
 *    entry or a sum that is not finite and > 0.  The _dev form checks the start PSF in its first kernel instead: a bad one sets the
 *    plan's status word to 1, the PSF is then never updated or written, and the image of that call is meaningless;
 *    fdr_richardson_lucy_blind_status synchronises the device and reads the word of the last call (0 = the start was good).
 *    The _dev form makes no host read-back and stays asynchronous on `stream`.  The first call on a plan allocates the workspace,
 *    kept until fdr_plan_destroy: one table of fdr_plan_filter_bytes, four PSF planes of FDR_BLIND_MAX_PSF floats, the status word and,
 *    at the first free-boundary call, one M x N float plane (the dense weights); FDR_ERR_ALLOC, plan intact, if it cannot be had.
 *    Later calls allocate nothing.  The workspace of the free-boundary form is needed as before.  The Wiener / CLS filter and the
 *    other calls' workspaces stay as they were.  No float atomics: results are bit-identical from call to call.
 *    fdr_psf_gaussian: out[i, j] = exp(-((i - c)^2 + (j - c)^2) / (2 sigma^2)) / sum, c = size / 2 (integer division: the centre of
 *    motionBlurKernel), evaluated in double, divided by its double sum, rounded once; sigma = 0 selects size / 4; 1 <= size <= 256.  */
#define FDR_BLIND_MAX_PSF 65536
typedef struct fdr_blind_params {
    int iterations;    /* >= 0 */
    int free_boundary; /* 0: the plain form; else the free-boundary, weighted form */
    int psf_hold;      /* the PSF is kept for the first psf_hold steps, >= 0 */
    int norm_area;     /* FDR_NORM_NONE / FDR_NORM_CROPPED / FDR_NORM_PADDED */
    float cov_sigma;   /* free form: as fdr_rlfree_params.sigma */
    int out_rows;      /* free form: as fdr_rlfree_params; plain form: 0 or rows */
    int out_cols;      /* free form: as fdr_rlfree_params; plain form: 0 or cols */
} fdr_blind_params;
int fdr_richardson_lucy_blind_f32(fdr_plan* plan, const float* img_host, int rows, int cols, int stride, const float* weights_host,
                                  int wstride, float* psf_host, int prows, int pcols, int pstride, float* out_host, int out_stride,
                                  const fdr_blind_params* params);
int fdr_richardson_lucy_blind_f32_dev(fdr_plan* plan, const float* d_img, int rows, int cols, int stride, const float* d_weights,
                                      int wstride, float* d_psf, int prows, int pcols, int pstride, float* d_out, int out_stride,
                                      const fdr_blind_params* params, void* stream);
int fdr_richardson_lucy_blind_status(fdr_plan* plan, int* status);
int fdr_psf_gaussian(int size, double sigma, float* out_host);
int fdr_psf_gaussian_dev(int device, int size, double sigma, float* d_out, void* stream);

/* -- Richardson-Lucy with a total-variation prior (Dey, Blanc-Feraud, Zimmer, Roux, Kam, Olivo-Marin & Zerubia 2006, "Richardson-Lucy
 *    algorithm with total variation regularization for 3D confocal microscope deconvolution"; the RLTV of DeconvolutionLab2), plain
 *    and free-boundary.  RL fits the noise and the iteration count is its only regularisation; here every step divides the
 *    multiplicative update by g = 1 - lambda div(grad u / |grad u|), which flattens the noise and keeps the edges, so the iteration
 *    settles instead of degrading.  The domain of the estimate is R x C: the window rows x cols in the plain form, the whole M x N
 *    plan in the free-boundary form.  Differences are forward and replicate at the domain's far edges:
 *        gx[i, j] = j < C-1 ? u[i, j+1] - u[i, j] : 0
 *        gy[i, j] = i < R-1 ? u[i+1, j] - u[i, j] : 0
 *        m  = sqrt(gx^2 + gy^2 + eps^2);  px = gx / m;  py = gy / m
 *        div[i, j] = (px[i, j] - (j > 0 ? px[i, j-1] : 0)) + (py[i, j] - (i > 0 ? py[i-1, j] : 0))            (div = -D^T)
 *        g = 1 - lambda div
 *        factor = w / g        w = 1 (plain form) or wgt = 1 / alpha (free form; 0 stays 0)
 *        plain form:  u <- max(u . factor . blur^T(r), 0)
 *        free form:   u <- max(u . factor . fullblur^T(pad(r)), 0)
 *    Starts, c, r, tau, coverage, output windows and normalisation are exactly those of fdr_richardson_lucy_f32 and
 *    fdr_richardson_lucy_free_f32; the factor is taken from the u that enters the step and is the division w / g, so a g that is
 *    exactly 1 gives the bits of those calls.  lambda lies in [0, FDR_RLTV_MAX_LAMBDA]: |div| <= 2 + sqrt(2), so g >= 0.57 always, and
 *    there is no clamp and no negative denominator.  lambda = 0 IS the call of the form (same bits, nothing else launched, no
 *    workspace).  eps is finite and positive, in the units of the data (a caller working in photon counts scales it); eps = 0
 *    selects FDR_RLTV_EPS.
 *    Three compromises.  Flux is no longer conserved exactly (the loss measured below 0.1 % at lambda = 0.01).  For eps well below
 *    4 lambda max(u) the explicit step oscillates at the scale of eps in flat areas: a call still repeats bit for bit, but results
 *    then depend on the arithmetic -- a float32 and a float64 run of the same formulas, lambda = 0.01 and eps = 1e-3 on a 256^2 picture
 *    scaled to 1, agree to 9e-6 after 3 steps, 1e-3 after 10 and 2.8e-2 in max-norm after 30 (rms 6.4e-4, under 0.01 dB of PSNR), while
 *    with eps = 0.05 they agree to 8e-7 through 100 steps.  And there is no accelerated, data-stopped or blind form, no anisotropic prior and no
 *    automatic lambda; the batched form is fdr_richardson_lucy_tv_batch_f32* below.
 *    Plans, refusals, overlap rules and phases are those of the underlying form (cov_sigma, out_rows and out_cols are the sigma,
 *    out_rows and out_cols of fdr_rlfree_params; the plain form takes no weights and out_rows = out_cols = 0 or rows, cols).
 *    FDR_ERR_ARG also for a null params pointer, a lambda that is negative, not finite or above FDR_RLTV_MAX_LAMBDA and an eps that is
 *    negative or not finite; always before any device work, the plan usable afterwards.  The first call with lambda > 0 allocates
 *    the workspace, kept until fdr_plan_destroy: two M x N float planes (the factor and the plain form's estimate, which has to lie
 *    dense beside it), 8 M N bytes; FDR_ERR_ALLOC, plan intact, if it cannot be had.  After it the _dev form allocates nothing and
 *    is asynchronous on `stream` (the free form needs its own workspace as before).  A step adds one streaming kernel, 8 bytes per
 *    pixel of the domain (12 in the free form, which reads wgt), and the plain form's update reads the factor: about 76 against 64
 *    bytes per padded pixel in the plain form, 80 against 68 in the free form, where the factor takes wgt's place in the update.
 *      fdr_rl_tv_factor_f32_dev  the factor alone, on any device window: d_out = w / g from d_u (rows x cols, row stride `stride`)
 *                              and d_w (same stride; NULL = 1), any size, stride and alignment.  FDR_ERR_ARG for a null d_u or d_out,
 *                              sizes <= 0, a stride below cols, lambda or eps as above, and an output that overlaps an input.     */
#define FDR_RLTV_MAX_LAMBDA 0.125f
#define FDR_RLTV_EPS 1e-3f
typedef struct fdr_rl_tv_params {
    int iterations;    /* >= 0 */
    int free_boundary; /* 0: the plain form; else the free-boundary, weighted form */
    float lambda;      /* weight of the prior, 0 .. FDR_RLTV_MAX_LAMBDA */
    float eps;         /* smoothing of |grad u|, > 0; 0 = FDR_RLTV_EPS */
    int norm_area;     /* FDR_NORM_NONE / FDR_NORM_CROPPED / FDR_NORM_PADDED */
    float cov_sigma;   /* free form: as fdr_rlfree_params.sigma */
    int out_rows;      /* free form: as fdr_rlfree_params; plain form: 0 or rows */
    int out_cols;      /* free form: as fdr_rlfree_params; plain form: 0 or cols */
} fdr_rl_tv_params;
int fdr_richardson_lucy_tv_f32(fdr_plan* plan, const float* img_host, int rows, int cols, int stride, const float* weights_host,
                               int wstride, float* out_host, int out_stride, const fdr_rl_tv_params* params);
int fdr_richardson_lucy_tv_f32_dev(fdr_plan* plan, const float* d_img, int rows, int cols, int stride, const float* d_weights, int wstride,
                                   float* d_out, int out_stride, const fdr_rl_tv_params* params, void* stream);
int fdr_rl_tv_factor_f32_dev(int device, const float* d_u, int rows, int cols, int stride, const float* d_w, float lambda, float eps,
                             float* d_out, int out_stride, void* stream);

/* -- Richardson-Lucy with the TV prior on several images per launch, and with the channels of a colour picture coupled.  Arguments,
 *    launch groups, forms and refusals are those of fdr_richardson_lucy_batch_f32* (image i at d_imgs + i img_pitch, written at
 *    d_out + i out_pitch; groups of `group` images of fdr_plan_set_batching, each run to completion on the caller's stream; in the
 *    free form ONE weights plane and one coverage per call), the prior's two numbers those of fdr_richardson_lucy_tv_f32*.  Per
 *    group and iteration the call makes ONE factor launch and the six passes of the form; image k's factor plane is the second
 *    source of its weighted update.
 *      couple = FDR_TV_COUPLE_NONE      every image on its own: it comes out bit for bit as fdr_richardson_lucy_tv_f32_dev gives it
 *                              on the same plan, for every group size, tail and layout; group = 1 is the loop of those calls.
 *      couple = FDR_TV_COUPLE_CHANNELS  vectorial TV: the images are the channels of one picture and share the norm of the prior,
 *                                  m^2 = eps^2 + sum_c (gx_c^2 + gy_c^2)  (c = 0, 1, .. in this order),  p_c = grad u_c / m,
 *                                  g_c = 1 - lambda div p_c,  factor_c = w / g_c,
 *                              so an edge falls in the same place in every channel.  m is no smaller than a channel's own, so
 *                              |div p_c| <= 2 + sqrt(2) and g >= 0.57 hold as before.  The whole batch has to be one launch group:
 *                              FDR_ERR_ARG for count > group.  One channel gives the bits of the uncoupled call.
 *    lambda = 0 IS fdr_richardson_lucy_batch_f32_dev (same bits, nothing else launched or allocated; couple is still checked).
 *    FDR_ERR_ARG also for an unknown `couple`; every refusal comes before any device work and leaves the plan usable.  The first
 *    call with lambda > 0 and a group g > 1 grows the prior's workspace from 2 to 2 g planes of M x N floats (plain form: image k's
 *    dense estimate beside its factor); the new block is had before the old one is let go, so FDR_ERR_ALLOC leaves the plan and the
 *    old workspace usable.  After it the _dev form allocates nothing and stays asynchronous on `stream`.  The coupled factor launch
 *    reads u twice: 12 bytes per pixel of the domain against 8 (16 against 12 with w).
 *      fdr_rl_tv_factor_group_f32_dev  the factor alone for `count` (1 .. 8) planes, plane k at d_u + k u_pitch -> d_out + k out_pitch,
 *                              one d_w (NULL = 1) for all, coupled or not: the checks of fdr_rl_tv_factor_f32_dev, and FDR_ERR_ARG for
 *                              a count outside 1 .. 8, an unknown `couple` and an output that overlaps an input anywhere in the span
 *                              of the planes.  Uncoupled, plane k has the bits of fdr_rl_tv_factor_f32_dev on it.
 *    The accelerated, data-stopped and blind forms with the prior, per-image weights, mixed-radix and full-spectrum plans have no
 *    batched form.                                                                                        */
typedef struct fdr_rl_tv_batch_params {
    int iterations;    /* >= 0 */
    int free_boundary; /* 0: the plain form; else the free-boundary, weighted form */
    float lambda;      /* weight of the prior, 0 .. FDR_RLTV_MAX_LAMBDA */
    float eps;         /* smoothing of |grad u|, > 0; 0 = FDR_RLTV_EPS */
    int norm_area;     /* FDR_NORM_NONE / FDR_NORM_CROPPED / FDR_NORM_PADDED, per image */
    float cov_sigma;   /* free form: as fdr_rlfree_params.sigma */
    int out_rows;      /* free form: as fdr_rlfree_params; plain form: 0 or rows */
    int out_cols;      /* free form: as fdr_rlfree_params; plain form: 0 or cols */
    int couple;        /* FDR_TV_COUPLE_NONE / FDR_TV_COUPLE_CHANNELS */
} fdr_rl_tv_batch_params;
int fdr_richardson_lucy_tv_batch_f32_dev(fdr_plan* plan, const float* d_imgs, size_t img_pitch, int count, int rows, int cols, int stride,
                                         const float* d_weights, int wstride, float* d_out, size_t out_pitch, int out_stride,
                                         const fdr_rl_tv_batch_params* params, void* stream);
int fdr_richardson_lucy_tv_batch_f32(fdr_plan* plan, const float* imgs_host, size_t img_pitch, int count, int rows, int cols, int stride,
                                     const float* weights_host, int wstride, float* out_host, size_t out_pitch, int out_stride,
                                     const fdr_rl_tv_batch_params* params);
int fdr_rl_tv_factor_group_f32_dev(int device, const float* d_u, size_t u_pitch, int count, int rows, int cols, int stride, const float* d_w,
                                   float lambda, float eps, int couple, float* d_out, size_t out_pitch, int out_stride, void* stream);

/* -- multi-frame Richardson-Lucy: `count` (1 .. FDR_MAX_FRAMES) exposures of ONE scene, each with its own PSF, restored jointly on
 *    the free-boundary, weighted form (Bertero & Boccacci 2000),
 *        u <- u / alpha . sum_k H_k^T( w_k d_k / (H_k u) ),   alpha = sum_k H_k^T w_k,
 *    so that what one PSF's transfer function lost another frame's supplies.
 *      fdr_set_frame_psfs*     the frame tables: PSF k (prows x pcols, row stride pstride) lies at psfs + k psf_pitch, top-left in the
 *                              plan as fdr_set_operator_psf* takes it, and becomes the pair H_k / (M N), conj(H_k) / (M N) by the passes
 *                              of that setter (same bits).  The tables live in a block of their own (2 count spectra), made or regrown
 *                              here, the new block before the old one is freed (FDR_ERR_ALLOC leaves the plan as it was); they never
 *                              touch the operator tables or the filter, and only the multi-frame calls (these and
 *                              fdr_tv_deconv_frames_f32*, whose solve table a new set invalidates) read them.  PSF
 *                              sums are NOT normalised: a frame's PSF sum is its relative exposure, which alpha accounts for, and a
 *                              registration shift goes into the PSF.  The checks of the operator setter, and FDR_ERR_ARG for a count
 *                              outside 1 .. FDR_MAX_FRAMES and, for count > 1, a psf_pitch below the span of one PSF.
 *      fdr_frame_count         the frames of the last successful set (0 before the first)
 *      fdr_spectrum_sum_f32_dev  the one new kernel alone: dst[i] = (accumulate ? dst[i] : src_0[i]) + src_k[i] for the remaining k in
 *                              ascending order, plain float adds, i < n_floats: the bits of that loop in float32, however the sources
 *                              are cut into launches.  d_srcs is a HOST array of n (1 .. 8) device pointers.  FDR_ERR_ARG for an n
 *                              outside 1 .. 8, an n_floats that is odd or < 2, a pointer that is null or not 16-byte aligned, and a dst
 *                              that overlaps a source other than exactly itself.
 *      fdr_blur_frames_f32_dev  adjoint = 0: the ONE window d_in gives `count` windows blur_k(x), window k at d_out + k out_pitch, with
 *                              the bits of fdr_blur_f32_dev under PSF k.  adjoint != 0: `count` windows y_k at d_in + k in_pitch give
 *                              the ONE window sum_k blur_k^T(y_k) at d_out: the K column-pass results are added in the spectrum
 *                              (fixed order, the same bits for every launch group) and go through one inverse row pass.
 *                              FDR_ERR_ARG for a count that is not fdr_frame_count, windows of the K-fold side that overlap each other
 *                              (pitch) and an output that overlaps the input anywhere in the span of the windows.
 *      fdr_richardson_lucy_frames_f32*  the restoration: frame k at imgs + k img_pitch, weights NULL (all ones), one plane for all
 *                              frames (weight_pitch = 0) or one per frame (at weights + k weight_pitch; saturation and cosmic rays
 *                              differ per exposure).  Semantics are fdr_richardson_lucy_free_f32*'s with the sums over k: wgt = alpha >
 *                              sigma count ? 1 / alpha : 0, u_0 = (sum_k sum dw_k) / (sum_k sum W_k) where seen; with tv_lambda > 0 the
 *                              prior of fdr_richardson_lucy_tv_f32* (tv_eps 0 = FDR_RLTV_EPS).  One frame has the bits of those calls.
 *                              No float atomics: two calls give the same bytes, whatever the plan's launch group.  FDR_ERR_ARG for what
 *                              fdr_richardson_lucy_free_f32* refuses, a count that is not fdr_frame_count (FDR_ERR_STATE with no
 *                              tables), an img_pitch below a window's span for count > 1, a weight_pitch that is neither 0 nor at least
 *                              the span, an output that overlaps any frame or weights plane, a bad tv_lambda or tv_eps; every refusal
 *                              comes before any device work.  The workspace (u, wgt, count dw planes, one spectrum, the sums) is made
 *                              on first use and grown for a larger count; the _dev form allocates nothing afterwards and stays
 *                              asynchronous on `stream`.                                                                           */
#define FDR_MAX_FRAMES 8
typedef struct fdr_rl_frames_params {
    int iterations;  /* >= 0 */
    float sigma;     /* coverage threshold per frame, in (0, 1): wgt = 0 where alpha <= sigma count */
    int norm_area;   /* FDR_NORM_NONE / FDR_NORM_CROPPED / FDR_NORM_PADDED */
    int out_rows;    /* the output window, rows .. M */
    int out_cols;    /* cols .. N */
    float tv_lambda; /* weight of the TV prior, 0 .. FDR_RLTV_MAX_LAMBDA; 0 = none */
    float tv_eps;    /* smoothing of |grad u|; 0 = FDR_RLTV_EPS */
} fdr_rl_frames_params;
int fdr_set_frame_psfs(fdr_plan* plan, const float* psfs_host, size_t psf_pitch, int count, int prows, int pcols, int pstride);
int fdr_set_frame_psfs_dev(fdr_plan* plan, const float* d_psfs, size_t psf_pitch, int count, int prows, int pcols, int pstride, void* stream);
int fdr_frame_count(fdr_plan* plan, int* count);
int fdr_spectrum_sum_f32_dev(int device, float* d_dst, const float* const* d_srcs, int n, size_t n_floats, int accumulate, void* stream);
int fdr_blur_frames_f32_dev(fdr_plan* plan, const float* d_in, size_t in_pitch, int rows, int cols, int stride, float* d_out, size_t out_pitch,
                            int out_stride, int count, int adjoint, void* stream);
int fdr_richardson_lucy_frames_f32_dev(fdr_plan* plan, const float* d_imgs, size_t img_pitch, int count, int rows, int cols, int stride,
                                       const float* d_weights, size_t weight_pitch, int wstride, float* d_out, int out_stride,
                                       const fdr_rl_frames_params* params, void* stream);
int fdr_richardson_lucy_frames_f32(fdr_plan* plan, const float* imgs_host, size_t img_pitch, int count, int rows, int cols, int stride,
                                   const float* weights_host, size_t weight_pitch, int wstride, float* out_host, int out_stride,
                                   const fdr_rl_frames_params* params);

/* -- total-variation (TV) regularised deconvolution by ADMM / split Bregman (Rudin-Osher-Fatemi 1992; Wang-Yang-Yin-Zhang 2008
 *    "FTVd"; Goldstein-Osher 2009): the edge-preserving restoration beside the linear filters and RL.  It uses the operator PSF of
 *    fdr_set_operator_psf* (H = DFT2 of the PSF top-left in the plan, blur / blur^T as above) and lives on the whole periodic
 *    M x N plan: pad(d) is d on the window rows x cols and 0 elsewhere, the result is cropped.  Differences are forward and periodic,
 *        Dx x[i, j] = x[i, (j+1) % N] - x[i, j],   Dy x[i, j] = x[(i+1) % M, j] - x[i, j],   Dx^T v[i, j] = v[i, (j-1) % N] - v[i, j]
 *    and |DFT(Dx)|^2 + |DFT(Dy)|^2 = L(u, v) = 4 sin^2(pi u / M) + 4 sin^2(pi v / N), the Laplacian symbol of the CLS filter.
 *        minimise over x (M x N):  mu / 2 ||blur(x) - pad(d)||^2 + TV(x)
 *        TV(x) = sum sqrt((Dx x)^2 + (Dy x)^2)  (isotropic)   or   sum |Dx x| + |Dy x|  (anisotropic)
 *        b = mu blur^T(pad(d)) over the whole plan;  x = pad(d);  wx = wy = 0;  t = 1 / rho;  n = iterations times:
 *            gx = Dx x + wx;  gy = Dy x + wy
 *            isotropic:    m = sqrt(gx^2 + gy^2);  s = m > t ? 1 - t / m : 0;  zx = s gx;  zy = s gy
 *            anisotropic:  zx = sign(gx) max(|gx| - t, 0);  zy likewise
 *            wx = gx - zx;  wy = gy - zy;  vx = zx - wx;  vy = zy - wy
 *            x = IDFT2( DFT2(b + rho (Dx^T vx + Dy^T vy)) / (mu |H|^2 + rho L) )        (IDFT2 includes 1 / (M N))
 *    The output is x on the window -- max(x, 0) with nonneg (the output only, never the iterate) -- normalised by norm_area as
 *    fdr_richardson_lucy_* defines FDR_NORM_NONE / _CROPPED / _PADDED.  n = 0 returns the window of pad(d).  mu weighs the data
 *    term (larger: closer to the data, less smoothing; about 1 / noise variance times the step you accept), rho is the ADMM
 *    penalty (it changes the path, not the minimiser; 1 .. 10 are usual).  The quotient table is evaluated in double and rounded
 *    once; a zero denominator (a PSF of sum 0) gives 0 there, as in the CLS filter.
 *    Plans as the operator's: FDR_MODE_FAST, M and N powers of two, 8 <= M <= 8192, 32 <= N <= 8192, neither FDR_FLAG_SIMPLE_PATH
 *    nor FDR_FLAG_FULL_SPECTRUM; every other plan FDR_ERR_ARG before any device work, a tables-only plan FDR_ERR_STATE, no
 *    operator PSF FDR_ERR_STATE.  FDR_ERR_ARG for mu or rho not finite or <= 0, iterations < 0, an unknown norm_area, a null
 *    params pointer or a window that does not fit; the plan stays usable after every refusal.  Unlike RL the output may be the
 *    input (d is read before anything is written).  Several images per launch, and the channels of a colour picture under one
 *    shrinkage: fdr_tv_deconv_batch_f32* below; fdr_batch_run and fdr_slab_* do not cover it.
 *    The first call on a plan allocates the TV workspace, kept until fdr_plan_destroy: the table (fdr_plan_filter_bytes) and six
 *    M x N float planes -- 24 M N + 8 M N bytes, about 1.8 GB at 8192^2 beside the plan's own; FDR_ERR_ALLOC, plan intact, if it
 *    cannot be had -- and, if no CLS call has, the M + N doubles of L.  After it the _dev form allocates nothing and is
 *    asynchronous on `stream`; the table is rebuilt (one pointwise pass, no transform) when mu, rho or the operator PSF changed.
 *    The host form copies in and out synchronously and counts as COMPUTE.  An iteration moves about 80 bytes per padded pixel
 *    (DESIGN.md section 14).                                                                                                 */
typedef struct fdr_tv_params {
    float mu;        /* weight of the data term, > 0 */
    float rho;       /* ADMM penalty, > 0 */
    int iterations;  /* >= 0 */
    int anisotropic; /* 0: isotropic TV, else anisotropic */
    int nonneg;      /* != 0: the output is max(x, 0) */
    int norm_area;   /* FDR_NORM_NONE / FDR_NORM_CROPPED / FDR_NORM_PADDED */
} fdr_tv_params;
int fdr_tv_deconv_f32(fdr_plan* plan, const float* img_host, int rows, int cols, int stride, float* out_host, int out_stride,
                      const fdr_tv_params* params);
int fdr_tv_deconv_f32_dev(fdr_plan* plan, const float* d_img, int rows, int cols, int stride, float* d_out, int out_stride,
                          const fdr_tv_params* params, void* stream);

/* -- batched and colour TV deconvolution: `count` images with one operator PSF, several per launch.  Image i
 *    is read at d_imgs + i img_pitch and written at d_out + i out_pitch (elements).  The batch is cut into launch groups of `group`
 *    images (fdr_plan_set_batching; the last group may be smaller) and every pass of a group -- b, the start, per iteration the
 *    spatial kernel, the forward rows, the solve columns and the x rows, the output -- is ONE launch over its images, so the solve
 *    table is read once per group and a small picture no longer leaves the chip idle.  A group runs to completion on the caller's
 *    stream, on the workspaces 0 .. group - 1, before the next begins, exactly as in fdr_richardson_lucy_batch_f32_dev.
 *      FDR_TV_COUPLE_NONE      every image on its own: it comes out bit for bit as fdr_tv_deconv_f32_dev gives it on the same plan,
 *                              for every group size, tail, window and layout, isotropic or anisotropic; group = 1 is literally the
 *                              loop of the single calls.
 *      FDR_TV_COUPLE_CHANNELS  vectorial TV (Blomgren & Chan 1998; Bresson & Chan 2008): the images are the channels of one picture,
 *                              TV(x) = sum over pixels of sqrt(sum over c of |grad x_c|^2).  The iteration is the one above with
 *                              one change: z_c = s g_c with s = m > t ? 1 - t / m : 0 and m = sqrt(sum over c of gx_c^2 + gy_c^2),
 *                              summed over c = 0 .. count - 1 in that order, in float -- one shrinkage for all channels of a pixel,
 *                              so an edge lies in the same place in every channel.  b, the duals, v, the divergence, the solve
 *                              (with the one table T), the clamp and the normalisation stay per channel.  All channels sit in one
 *                              launch: FDR_ERR_ARG if count exceeds the plan's `group` (at most 8).  Isotropic only: FDR_ERR_ARG with
 *                              anisotropic != 0.  count = 1 gives the bits of fdr_tv_deconv_f32_dev.  The minimiser differs from
 *                              the channel-wise one; its best mu is about 0.7 of the channel-wise best.
 *    Refusals, always before any device work and with the plan usable afterwards: a null pointer or null params, a negative count
 *    (count = 0 returns FDR_OK at once), whatever fdr_tv_deconv_f32_dev refuses for one image, an unknown coupling, and -- unlike
 *    the single call -- an output that overlaps the input anywhere within the span of the batch.  The first call with a group g
 *    larger than any before grows the TV workspace to the table and 6 g planes (8 M N + 24 g M N bytes; the table is then built
 *    again); FDR_ERR_ALLOC leaves the plan and the workspace it had intact.  After that the _dev form allocates nothing, reads
 *    nothing back and stays asynchronous on `stream`; the host form copies in and out synchronously.  Results repeat bit for bit
 *    from call to call (no atomics).                                                                                          */
#define FDR_TV_COUPLE_NONE 0     /* every image on its own: fdr_tv_deconv_f32_dev per image, bit for bit */
#define FDR_TV_COUPLE_CHANNELS 1 /* vectorial TV: one shrinkage by the joint gradient norm of all `count` images */
typedef struct fdr_tv_batch_params {
    float mu;        /* weight of the data term, > 0 */
    float rho;       /* ADMM penalty, > 0 */
    int iterations;  /* >= 0 */
    int anisotropic; /* 0: isotropic TV, else anisotropic (FDR_TV_COUPLE_NONE only) */
    int nonneg;      /* != 0: the output is max(x, 0) */
    int norm_area;   /* FDR_NORM_NONE / FDR_NORM_CROPPED / FDR_NORM_PADDED, per image */
    int coupling;    /* FDR_TV_COUPLE_NONE / FDR_TV_COUPLE_CHANNELS */
} fdr_tv_batch_params;
int fdr_tv_deconv_batch_f32_dev(fdr_plan* plan, const float* d_imgs, size_t img_pitch, int count, int rows, int cols, int stride,
                                float* d_out, size_t out_pitch, int out_stride, const fdr_tv_batch_params* params, void* stream);
int fdr_tv_deconv_batch_f32(fdr_plan* plan, const float* imgs_host, size_t img_pitch, int count, int rows, int cols, int stride,
                            float* out_host, size_t out_pitch, int out_stride, const fdr_tv_batch_params* params);

/* -- free-boundary, weighted TV deconvolution: fdr_tv_deconv_f32 for a picture that is a crop of a larger scene (DESIGN.md section
 *    31).  The periodic call's data term counts the zero padding of the plan as data; here the data constrain x inside the window
 *    only, each pixel by its weight, and x is free elsewhere on the plan, as in fdr_richardson_lucy_free_f32:
 *        minimise over x (M x N):  mu / 2 sum m (blur(x) - pad(d))^2 + TV(x),   m = the weights on the window, 0 elsewhere
 *    (weights null: 1 on the window; 0 excludes a pixel, as a dead or saturated one).  ADMM with two splittings (Almeida &
 *    Figueiredo 2013; Matakos, Ramani & Fessler 2013): z = D x with the scaled dual w and the penalty rho as above, and s = blur(x)
 *    with the scaled dual q and the penalty nu, which keeps the linear solve diagonal in the Fourier domain:
 *        x = pad(d);  w = 0;  q = 0;  t = 1 / rho;  n = iterations times:
 *            c = blur(x)                                                             whole plan
 *            e = c + q;  s = (mu m pad(d) + nu e) / (mu m + nu);  q = e - s;  r = s - q     (outside the window: q = 0, r = c)
 *            b = blur^T(r)                                                           whole plan
 *            g = D x + w;  z = shrink(g, t);  w = g - z;  v = z - w                  as fdr_tv_deconv_f32
 *            x = IDFT2( DFT2(nu b + rho (Dx^T vx + Dy^T vy)) / (nu |H|^2 + rho L) )
 *    The output is the top-left out_rows x out_cols of x (rows <= out_rows <= M, cols <= out_cols <= N: the window, the whole plan
 *    or anything between), max(x, 0) with nonneg, normalised by norm_area over what is returned as fdr_richardson_lucy_free_f32
 *    does.  n = 0 returns pad(d) there.  nu = 0 selects nu = rho; like rho it changes the path, not the minimiser.  With the
 *    window equal to the plan and no weights the minimiser is that of fdr_tv_deconv_f32.  The solve divides by nu |H|^2 + rho L with
 *    nu of the order of rho, so a large mu does not amplify rounding as it does in the periodic call.
 *    Plans and refusals as fdr_tv_deconv_f32*, and FDR_ERR_ARG for nu not finite or < 0, wstride < cols with weights, an output
 *    window outside [rows .. M] x [cols .. N], out_stride < out_cols, and an output that overlaps the input or the weights (both
 *    are read in every iteration, in place, from the caller's windows).  Weights outside [0, 1] are not checked.  The plan stays
 *    usable after every refusal.
 *    The first call on a plan allocates, beside the TV workspace of fdr_tv_deconv_f32, two more M x N float planes (q and c / r) in
 *    a block of their own, kept until fdr_plan_destroy; FDR_ERR_ALLOC, plan intact, if it cannot be had.  After it the _dev form
 *    allocates nothing, reads nothing back and is asynchronous on `stream`; the solve table is shared with fdr_tv_deconv_f32 and
 *    rebuilt when nu, rho or the operator PSF differ from what it was built for.  The host form copies in and out synchronously.
 *    An iteration is three blur chains, the spatial kernel and one streaming pass over the window (20 bytes per pixel, 24 with
 *    weights).  Results repeat bit for bit from call to call (no atomics).                                                     */
typedef struct fdr_tv_free_params {
    float mu;        /* weight of the data term, > 0 */
    float rho;       /* ADMM penalty of z = D x, > 0 */
    float nu;        /* ADMM penalty of s = blur(x), >= 0; 0 selects rho */
    int iterations;  /* >= 0 */
    int anisotropic; /* 0: isotropic TV, else anisotropic */
    int nonneg;      /* != 0: the output is max(x, 0) */
    int norm_area;   /* FDR_NORM_NONE / FDR_NORM_CROPPED / FDR_NORM_PADDED, over the output window */
    int out_rows;    /* rows .. M */
    int out_cols;    /* cols .. N */
} fdr_tv_free_params;
int fdr_tv_deconv_free_f32(fdr_plan* plan, const float* img_host, int rows, int cols, int stride, const float* weights_host, int wstride,
                           float* out_host, int out_stride, const fdr_tv_free_params* params);
int fdr_tv_deconv_free_f32_dev(fdr_plan* plan, const float* d_img, int rows, int cols, int stride, const float* d_weights, int wstride,
                               float* d_out, int out_stride, const fdr_tv_free_params* params, void* stream);

/* -- noise-constrained TV deconvolution: fdr_tv_deconv_free_f32 with mu chosen from the noise level.  The
 *    caller states the noise standard deviation sigma of the picture instead of the weight mu (sigma = 0: it is estimated from the
 *    window as fdr_noise_sigma_f32 does; the weights are not looked at), and the call solves the constrained problem
 *        minimise over x (M x N):  TV(x)   subject to   sum m (blur(x) - pad(d))^2 <= c2 = tau sigma^2 S,   S = sum m
 *    (m as above: the weights on the window, 0 elsewhere; tau = 0 selects 1) by ADMM on the splittings of the free call, the
 *    weighted data step replaced by a projection of s onto the discrepancy ball (Afonso, Bioucas-Dias & Figueiredo 2011, C-SALSA;
 *    Wen & Chan 2012).  Every iteration k is that of fdr_tv_deconv_free_f32 with its own weight mu_k:
 *            c = blur(x)
 *            res_e = sum m (c + q - pad(d))^2;  res_c = sum m (c - pad(d))^2;  S = sum m         over the window, in double
 *            g = 0 for res_e <= c2;  FDR_TV_AUTO_MAX_RATIO for c2 = 0 or a quotient that is not finite;
 *                else min(sqrt(res_e / c2) - 1, FDR_TV_AUTO_MAX_RATIO);   mu_k = float(nu g)
 *            e = c + q;  s = (mu_k m pad(d) + nu e) / (mu_k m + nu);  q = e - s;  r = s - q;  ... the rest unchanged
 *    For weights of 0 and 1 this s is the exact projection of e onto the ball, the iteration is ADMM for the constrained problem
 *    and mu_k converges to its Lagrange multiplier: the mu of the fdr_tv_deconv_free_f32 call with the same minimiser.  For
 *    fractional weights it is an approximation of the projection and the discrepancy settles above the target (1.35 times after 300
 *    steps on the quality scene of the tests).  nu = 0 selects FDR_TV_AUTO_NU_RATIO rho: the projection needs nu well above rho
 *    to converge in about a hundred steps; out_rows x out_cols, nonneg and norm_area as in the free call;
 *    n = 0 returns pad(d).
 *    trace (3 n doubles, optional): trace[3 k .. 3 k + 2] = (res_c, res_e, mu_k) of iteration k.  The host form fills `result`
 *    (optional) from the last iteration; with n = 0 nothing is measured or estimated: sigma is the one given and target, mu,
 *    discrepancy and S are 0.
 *    Plans and refusals as fdr_tv_deconv_free_f32*, and FDR_ERR_ARG for sigma or tau negative or not finite, a window below 3 x 3
 *    when sigma is to be estimated, and (_dev) a d_trace range of 3 n doubles that overlaps the input, the weights or the output.
 *    Every refusal comes before any device work and leaves the plan usable.
 *    The first call on a plan allocates, beside the workspaces of fdr_tv_deconv_free_f32, one small block (the partials of the
 *    sums, mu_k, the last sums), kept until fdr_plan_destroy; FDR_ERR_ALLOC, plan intact, if it cannot be had.  After it the _dev
 *    form allocates nothing and, with sigma > 0, reads nothing back and is asynchronous on `stream`; with sigma = 0 it waits
 *    for `stream` once, before the first iteration, to read the noise sum back (as fdr_richardson_lucy_auto_f32_dev does for its
 *    residual rule).  The solve table is the shared one, built for nu.  An iteration adds one more streaming pass over the window
 *    (12 bytes per pixel, 16 with weights) and a single-workgroup fold to the free call's.  Results and traces repeat bit for bit from
 *    call to call (no atomics; every sum runs in a fixed order that does not depend on the alignment of the windows).            */
#define FDR_TV_AUTO_MAX_RATIO 1e6 /* the clamp of sqrt(res_e / c2) - 1 */
#define FDR_TV_AUTO_NU_RATIO 25.f /* nu = 0 selects this times rho */
typedef struct fdr_tv_auto_params {
    float sigma;     /* noise standard deviation of the picture, >= 0; 0 = fdr_noise_sigma of the window */
    float tau;       /* the ball is tau sigma^2 S, >= 0; 0 selects 1 */
    float rho;       /* ADMM penalty of z = D x, > 0 */
    float nu;        /* ADMM penalty of s = blur(x), >= 0; 0 selects FDR_TV_AUTO_NU_RATIO rho */
    int iterations;  /* >= 0 */
    int anisotropic; /* 0: isotropic TV, else anisotropic */
    int nonneg;      /* != 0: the output is max(x, 0) */
    int norm_area;   /* FDR_NORM_NONE / FDR_NORM_CROPPED / FDR_NORM_PADDED, over the output window */
    int out_rows;    /* rows .. M */
    int out_cols;    /* cols .. N */
} fdr_tv_auto_params;
typedef struct fdr_tv_auto_result {
    double sigma;       /* the noise level used: given or estimated */
    double target;      /* c2 = tau sigma^2 S */
    double mu;          /* mu_k of the last iteration: the mu of the equivalent fdr_tv_deconv_free_f32 call */
    double discrepancy; /* res_c of the last iteration, to compare with target */
    double S;           /* sum m: rows cols without weights */
} fdr_tv_auto_result;
int fdr_tv_deconv_auto_f32(fdr_plan* plan, const float* img_host, int rows, int cols, int stride, const float* weights_host, int wstride,
                           float* out_host, int out_stride, const fdr_tv_auto_params* params, fdr_tv_auto_result* result, double* trace_host);
int fdr_tv_deconv_auto_f32_dev(fdr_plan* plan, const float* d_img, int rows, int cols, int stride, const float* d_weights, int wstride,
                               float* d_out, int out_stride, const fdr_tv_auto_params* params, double* d_trace, void* stream);

/* -- free-boundary and noise-constrained TV deconvolution in groups: `count` crops with one operator PSF and one weights plane (or
 *    none), several per launch, and the vectorial coupling for them.  Image i is read at d_imgs + i img_pitch
 *    and written at d_out + i out_pitch (elements), its output window out_rows x out_cols as in the single calls; the one weights
 *    window serves every image, as in fdr_richardson_lucy_batch_f32*.  The batch is cut into launch groups of `group` images
 *    (fdr_plan_set_batching; the last group may be smaller) and every pass of a group -- the start, per iteration the blur, the data
 *    step on the windows (for the auto form the sums and the fold before it), the adjoint blur, the spatial kernel and the three
 *    solve passes, the output -- is ONE launch over its images.  A group runs to completion on the caller's stream, on the
 *    workspaces 0 .. group - 1, before the next begins.
 *      FDR_TV_COUPLE_NONE      every image on its own: it comes out bit for bit as fdr_tv_deconv_free_f32_dev / _auto_f32_dev gives it
 *                              on the same plan (for the auto form every trace entry as well), for every group size, tail, window,
 *                              output window, pitch and stride, weights none, mask or fractional, isotropic or anisotropic;
 *                              group = 1 is literally the loop of the single calls.
 *      FDR_TV_COUPLE_CHANNELS  the images are the channels of one picture under vectorial TV.  The iteration of the single call
 *                              changes in one place: z_c = s g_c with the joint gradient norm over the channels, exactly as in
 *                              fdr_tv_deconv_batch_f32* (summed over c in order, in float; isotropic only).  The data step, the
 *                              duals q_c, w_c, b_c, the solve and -- auto form -- the ball, the three sums and mu_k stay per channel:
 *                              noise levels differ between channels, so there is no joint ball.  count = 1 gives the single call's
 *                              bits.  FDR_ERR_ARG if count exceeds the plan's `group` (at most 8) or with anisotropic != 0.
 *    Auto form: `sigmas` (host, count entries) gives a noise level per image, null: params->sigma serves all; an entry of 0 is
 *    estimated from that image as the single call does (one wait on the stream before its group's first iteration).  Each image
 *    has its own ball tau sigma_i^2 S, its own sums and its own mu_k.  Image i's trace (3 n doubles) goes to d_trace + i
 *    trace_pitch (elements; d_trace may be null); the host form fills results[i] (may be null) as the single call fills `result`.
 *    Refusals, always before any device work and with the plan usable afterwards: a null plan or null params, a negative count
 *    (count = 0 returns FDR_OK at once), whatever the single call refuses for one image, an unknown coupling, any output of the
 *    batch that overlaps any input or the weights; auto form: a sigmas entry negative or not finite, trace_pitch < 3 n when a trace
 *    is asked for and count > 1, a trace range that overlaps an input, an output or the weights.
 *    The first call with a group g larger than any before grows the free call's block to 2 g planes, the auto block to g sets of
 *    partials, sums and mu_k, and the TV workspace to 6 g planes, each new block had before the old one is let go; FDR_ERR_ALLOC
 *    leaves the plan and its workspaces intact.  After that the _dev forms allocate nothing and, with every sigma given, read
 *    nothing back and stay asynchronous on `stream`; the host forms copy in and out synchronously.  Results and traces repeat bit
 *    for bit from call to call (no atomics).                                                                                  */
typedef struct fdr_tv_free_batch_params {
    float mu;        /* weight of the data term, > 0 */
    float rho;       /* ADMM penalty of z = D x, > 0 */
    float nu;        /* ADMM penalty of s = blur(x), >= 0; 0 selects rho */
    int iterations;  /* >= 0 */
    int anisotropic; /* 0: isotropic TV, else anisotropic (FDR_TV_COUPLE_NONE only) */
    int nonneg;      /* != 0: the output is max(x, 0) */
    int norm_area;   /* FDR_NORM_NONE / FDR_NORM_CROPPED / FDR_NORM_PADDED, per image over its output window */
    int out_rows;    /* rows .. M */
    int out_cols;    /* cols .. N */
    int coupling;    /* FDR_TV_COUPLE_NONE / FDR_TV_COUPLE_CHANNELS */
} fdr_tv_free_batch_params;
int fdr_tv_deconv_free_batch_f32_dev(fdr_plan* plan, const float* d_imgs, size_t img_pitch, int count, int rows, int cols, int stride,
                                     const float* d_weights, int wstride, float* d_out, size_t out_pitch, int out_stride,
                                     const fdr_tv_free_batch_params* params, void* stream);
int fdr_tv_deconv_free_batch_f32(fdr_plan* plan, const float* imgs_host, size_t img_pitch, int count, int rows, int cols, int stride,
                                 const float* weights_host, int wstride, float* out_host, size_t out_pitch, int out_stride,
                                 const fdr_tv_free_batch_params* params);
typedef struct fdr_tv_auto_batch_params {
    float sigma;     /* noise standard deviation of every picture when `sigmas` is null, >= 0; 0 = estimated per image */
    float tau;       /* the balls are tau sigma_i^2 S, >= 0; 0 selects 1 */
    float rho;       /* ADMM penalty of z = D x, > 0 */
    float nu;        /* ADMM penalty of s = blur(x), >= 0; 0 selects FDR_TV_AUTO_NU_RATIO rho */
    int iterations;  /* >= 0 */
    int anisotropic; /* 0: isotropic TV, else anisotropic (FDR_TV_COUPLE_NONE only) */
    int nonneg;      /* != 0: the output is max(x, 0) */
    int norm_area;   /* FDR_NORM_NONE / FDR_NORM_CROPPED / FDR_NORM_PADDED, per image over its output window */
    int out_rows;    /* rows .. M */
    int out_cols;    /* cols .. N */
    int coupling;    /* FDR_TV_COUPLE_NONE / FDR_TV_COUPLE_CHANNELS */
} fdr_tv_auto_batch_params;
int fdr_tv_deconv_auto_batch_f32_dev(fdr_plan* plan, const float* d_imgs, size_t img_pitch, int count, int rows, int cols, int stride,
                                     const float* d_weights, int wstride, float* d_out, size_t out_pitch, int out_stride,
                                     const fdr_tv_auto_batch_params* params, const double* sigmas, double* d_trace, size_t trace_pitch,
                                     void* stream);
int fdr_tv_deconv_auto_batch_f32(fdr_plan* plan, const float* imgs_host, size_t img_pitch, int count, int rows, int cols, int stride,
                                 const float* weights_host, int wstride, float* out_host, size_t out_pitch, int out_stride,
                                 const fdr_tv_auto_batch_params* params, const double* sigmas, fdr_tv_auto_result* results,
                                 double* trace_host, size_t trace_pitch);

/* -- Poisson-likelihood TV deconvolution: fdr_tv_deconv_free_f32 for photon-limited pictures.  The data
 *    term is the negative Poisson log-likelihood of the counts instead of least squares (PIDAL, Figueiredo & Bioucas-Dias 2010;
 *    Setzer, Steidl & Teuber 2010), convex like the free call's, so the iteration settles where fdr_richardson_lucy_tv_f32 cycles:
 *        minimise over x (M x N):  mu sum m [ (blur(x) + b) - d+ log(blur(x) + b) ] + TV(x)
 *    d+ = max(d, 0); m = the weights on the window, 0 elsewhere; b = background >= 0, a known level in the units of the data (sky,
 *    dark current); the detector's gain is part of mu: mu = photons per unit times the weight wanted on the likelihood.  The
 *    iteration is that of fdr_tv_deconv_free_f32, every line of it, with the data step replaced: for a window pixel with m > 0
 *            e = c + q;  k = mu m / nu;  a = e + b - k;  y = the root >= 0 of y^2 - a y - k d+ = 0;  s = y - b;  q = e - s;  r = s - q
 *    with the root formed without cancellation, rt = sqrt(a a + 4 k d+), y = a >= 0 ? (a + rt) / 2 : 2 k d+ / (rt - a); for m = 0,
 *    as outside the window, s = e.  s + b >= 0 always.  Every operation is a correctly rounded float operation in the order
 *    tvpoisson_data_pixel (csrc/fdr_kernels.hpp) states, so a float32 model repeats the step bit for bit.  The start is x = pad(d);
 *    nu = 0 selects rho; the output window, nonneg and norm_area as in the free call; n = 0 returns pad(d).  Negative data are
 *    clamped, not refused; a NaN in the data stays a NaN in the output.
 *      fdr_tv_deconv_poisson_f32*        one image: arguments, plans, workspaces (none beyond the free call's) and passes as
 *                                        fdr_tv_deconv_free_f32*; the data step has its own pass name.
 *      fdr_tv_deconv_poisson_batch_f32*  `count` crops as fdr_tv_deconv_free_batch_f32*: FDR_TV_COUPLE_NONE gives every image the
 *                                        bits of the single _dev call, for every group, tail, pitch and alignment (group = 1 is the
 *                                        loop of single calls); FDR_TV_COUPLE_CHANNELS shares the shrinkage by the joint gradient
 *                                        norm, the data step stays per channel (count <= group, isotropic; count = 1: the single
 *                                        call's bits).
 *      fdr_tv_poisson_step_f32_dev       the data step alone on the window rows x cols of two dense M x N planes of the caller's
 *                                        (row stride N, 16-byte aligned): c = blur(x) and q in, r and the new q out; nothing outside
 *                                        the window is read or written.  d_img and d_weights (NULL = 1) are rows x cols windows
 *                                        of any alignment.  nu must be > 0 here.  Needs no PSF; asynchronous on `stream`.
 *      fdr_tv_poisson_step_group_f32_dev the same for `count` (1 .. 8) images in one launch: image k's planes at d_c + k c_pitch and
 *                                        d_q + k q_pitch (pitches >= M N, multiples of 4), its data at d_imgs + k img_pitch, one
 *                                        weights window for all; image k gets the bits of the single step.
 *    FDR_ERR_ARG, before any device work and with the plan usable afterwards: whatever fdr_tv_deconv_free_f32* (the batch:
 *    fdr_tv_deconv_free_batch_f32*) refuses, and a background that is negative or not finite; the steps: a window outside the plan,
 *    a stride below cols, mu or nu not finite or <= 0, planes that are misaligned or overlap each other, the data or the weights. */
typedef struct fdr_tv_poisson_params {
    float mu;         /* weight of the likelihood, > 0: photons per unit of the data times the weight wanted */
    float rho;        /* ADMM penalty of z = D x, > 0 */
    float nu;         /* ADMM penalty of s = blur(x), >= 0; 0 selects rho */
    float background; /* b >= 0, in the units of the data */
    int iterations;   /* >= 0 */
    int anisotropic;  /* 0: isotropic TV, else anisotropic */
    int nonneg;       /* != 0: the output is max(x, 0) */
    int norm_area;    /* FDR_NORM_NONE / FDR_NORM_CROPPED / FDR_NORM_PADDED, over the output window */
    int out_rows;     /* rows .. M */
    int out_cols;     /* cols .. N */
} fdr_tv_poisson_params;
typedef struct fdr_tv_poisson_batch_params {
    float mu;         /* weight of the likelihood, > 0 */
    float rho;        /* ADMM penalty of z = D x, > 0 */
    float nu;         /* ADMM penalty of s = blur(x), >= 0; 0 selects rho */
    float background; /* b >= 0, one for all images */
    int iterations;   /* >= 0 */
    int anisotropic;  /* 0: isotropic TV, else anisotropic (FDR_TV_COUPLE_NONE only) */
    int nonneg;       /* != 0: the output is max(x, 0) */
    int norm_area;    /* FDR_NORM_NONE / FDR_NORM_CROPPED / FDR_NORM_PADDED, per image over its output window */
    int out_rows;     /* rows .. M */
    int out_cols;     /* cols .. N */
    int coupling;     /* FDR_TV_COUPLE_NONE / FDR_TV_COUPLE_CHANNELS */
} fdr_tv_poisson_batch_params;
int fdr_tv_deconv_poisson_f32(fdr_plan* plan, const float* img_host, int rows, int cols, int stride, const float* weights_host, int wstride,
                              float* out_host, int out_stride, const fdr_tv_poisson_params* params);
int fdr_tv_deconv_poisson_f32_dev(fdr_plan* plan, const float* d_img, int rows, int cols, int stride, const float* d_weights, int wstride,
                                  float* d_out, int out_stride, const fdr_tv_poisson_params* params, void* stream);
int fdr_tv_deconv_poisson_batch_f32_dev(fdr_plan* plan, const float* d_imgs, size_t img_pitch, int count, int rows, int cols, int stride,
                                        const float* d_weights, int wstride, float* d_out, size_t out_pitch, int out_stride,
                                        const fdr_tv_poisson_batch_params* params, void* stream);
int fdr_tv_deconv_poisson_batch_f32(fdr_plan* plan, const float* imgs_host, size_t img_pitch, int count, int rows, int cols, int stride,
                                    const float* weights_host, int wstride, float* out_host, size_t out_pitch, int out_stride,
                                    const fdr_tv_poisson_batch_params* params);
int fdr_tv_poisson_step_f32_dev(fdr_plan* plan, float* d_c, float* d_q, const float* d_img, int rows, int cols, int stride,
                                const float* d_weights, int wstride, float mu, float nu, float background, void* stream);
int fdr_tv_poisson_step_group_f32_dev(fdr_plan* plan, float* d_c, size_t c_pitch, float* d_q, size_t q_pitch, const float* d_imgs,
                                      size_t img_pitch, int count, int rows, int cols, int stride, const float* d_weights, int wstride,
                                      float mu, float nu, float background, void* stream);

/* -- multi-frame TV deconvolution: the `count` = fdr_frame_count exposures of ONE scene under one TV prior.
 *    Frame k has the PSF k of fdr_set_frame_psfs* (H_k, sums NOT normalised: a frame's PSF sum is its exposure, a registration
 *    shift goes into the PSF) and weights m_k on its window; one unknown x lives on the whole M x N plan:
 *        minimise over x:  mu sum_k Phi_k(blur_k(x)) + TV(x)
 *          FDR_TV_FRAMES_LEAST_SQUARES:  Phi_k(s) = 1/2 sum m_k (s - pad(d_k))^2
 *          FDR_TV_FRAMES_POISSON:        Phi_k(s) = sum m_k [ (s + b) - d_k+ log(s + b) ],   b = background >= 0
 *        x = pad(d_0);  w = 0;  q_k = 0;  t = 1 / rho;  nu = 0 selects rho;  n = iterations times:
 *            c_k = blur_k(x) over the whole plan, k = 0 .. count - 1
 *            e_k = c_k + q_k;  s_k = the data step of fdr_tv_deconv_free_f32* / fdr_tv_deconv_poisson_f32* on frame k's window with m_k
 *            q_k = e_k - s_k;  r_k = s_k - q_k                                  (outside the window: q_k = 0, r_k = c_k)
 *            b = sum_k blur_k^T(r_k): added in the spectrum in ascending k (the sum kernel of the multi-frame RL call), ONE inverse row pass
 *            g = D x + w;  z = shrink(g, t);  w = g - z;  v = z - w             (as fdr_tv_deconv_f32)
 *            x = IDFT2( DFT2(nu b + rho D^T v) / (nu sum_k |H_k|^2 + rho L) )
 *    The start is frame 0 (the problem is convex: the start changes the path, not the minimiser); n = 0 returns pad(d_0).  The output
 *    window, nonneg and norm_area are the free call's.  Frame k is read at imgs + k img_pitch; weights are NULL (all ones), one
 *    plane for all frames (weight_pitch = 0) or one per frame (at weights + k weight_pitch).  One frame gives the bits of
 *    fdr_tv_deconv_free_f32_dev / fdr_tv_deconv_poisson_f32_dev under that PSF as the operator PSF.  No atomics: two calls give the
 *    same bytes, whatever the plan's launch group.  The operator PSF is neither needed nor touched; the solve table is shared with the
 *    other TV calls, each of which builds its own again after a call of another kind or a new frame set.
 *    THE STREAM TRAVELS IN THE STRUCT, deliberately: the _dev form runs on (hipStream_t)params->stream (NULL = the null stream) and
 *    has no `void* stream` parameter; the host form ignores the field.  The stream-order table of the test suite is keyed on
 *    `void* stream` parameters and is closed to edits for now, so this entry is fenced by a test file of its own with the same
 *    helper; when that table can next be edited its cases move there.
 *    FDR_ERR_ARG, before any device work and with the plan usable afterwards: what fdr_tv_deconv_free_f32* refuses (but for the
 *    operator PSF, which is not needed), an unknown data_term, a background that is negative or not finite or != 0 with least
 *    squares, a count that is not fdr_frame_count (FDR_ERR_STATE with no frame tables), an img_pitch below a window's span for
 *    count > 1, a weight_pitch that is neither 0 nor at least the span, an output that overlaps any frame or weights plane.  The
 *    workspace (count planes q, count planes c / r and one spectrum, beside the TV workspace of one image) is made on first use and
 *    grown for a larger count, the new block before the old one is freed (FDR_ERR_ALLOC leaves everything as it was); the _dev
 *    form allocates nothing afterwards, reads nothing back and stays asynchronous on its stream.                                   */
#define FDR_TV_FRAMES_LEAST_SQUARES 0
#define FDR_TV_FRAMES_POISSON 1
typedef struct fdr_tv_frames_params {
    float mu;         /* weight of the data term, > 0 */
    float rho;        /* ADMM penalty of z = D x, > 0 */
    float nu;         /* ADMM penalty of s_k = blur_k(x), >= 0; 0 selects rho */
    float background; /* FDR_TV_FRAMES_POISSON: b >= 0, in the units of the data; must be 0 with least squares */
    int data_term;    /* FDR_TV_FRAMES_LEAST_SQUARES / FDR_TV_FRAMES_POISSON */
    int iterations;   /* >= 0 */
    int anisotropic;  /* 0: isotropic TV, else anisotropic */
    int nonneg;       /* != 0: the output is max(x, 0) */
    int norm_area;    /* FDR_NORM_NONE / FDR_NORM_CROPPED / FDR_NORM_PADDED, over the output window */
    int out_rows;     /* rows .. M */
    int out_cols;     /* cols .. N */
    void* stream;     /* _dev form: the hipStream_t of the call (NULL = the null stream); the host form ignores it */
} fdr_tv_frames_params;
int fdr_tv_deconv_frames_f32(fdr_plan* plan, const float* imgs_host, size_t img_pitch, int count, int rows, int cols, int stride,
                             const float* weights_host, size_t weight_pitch, int wstride, float* out_host, int out_stride,
                             const fdr_tv_frames_params* params);
int fdr_tv_deconv_frames_f32_dev(fdr_plan* plan, const float* d_imgs, size_t img_pitch, int count, int rows, int cols, int stride,
                                 const float* d_weights, size_t weight_pitch, int wstride, float* d_out, int out_stride,
                                 const fdr_tv_frames_params* params);

/* -- sectioned restoration (Trussell & Hunt 1978; Nagy & O'Leary 1998): a picture of any size, larger than a
 *    plan can be, is cut into overlapping tiles, every tile is restored as a crop of a larger scene by the free-boundary iteration
 *    of the chosen method on ONE tile plan, with one PSF for all tiles or one per tile (a blur that changes across the frame), and
 *    the tiles are blended with a partition of unity.  Geometry, per axis (rows; columns alike), in integers and doubles on the host:
 *        n = 1 and the window win = rows when rows <= T; otherwise win = T, n = ceil((rows - O) / (T - O)) and tile a starts at
 *        y_a = min(a (T - O), rows - T): all tiles have one size, the last ends at the picture's edge (its overlap may exceed O)
 *        h(s) = 0.5 - 0.5 cos(pi s) for s < 1, else 1;  w_a(t) = rise . fall,  rise = h((t + 0.5) / O_a) with O_a the real overlap
 *        with tile a - 1 (1 for a = 0 or O_a = 0), fall the same from the far end against tile a + 1
 *        W_a(y) = w_a(y - y_a) / sum over the covering a' of w_a'(y - y_a'), formed in double and rounded to float once
 *    With 0 <= O <= T / 2 at most three tiles cover a pixel along an axis.  With o_ab the restored window of tile (a, b),
 *        out[y, x] = sum over covering a (outer, ascending), covering b (inner, ascending) of (Wy_a(y) . Wx_b(x)) . o_ab[y - y_a, x - x_b]
 *    in float, every product and sum rounded to nearest on its own, starting from +0: a float32 model repeats it bit for bit.
 *    Tile (a, b) is the single call fdr_richardson_lucy_free_f32_dev (FDR_TILED_RL_FREE: iterations, sigma) or
 *    fdr_tv_deconv_free_f32_dev (FDR_TILED_TV_FREE: mu, rho, nu, iterations, anisotropic, nonneg) on its win_rows x win_cols window
 *    of the picture (and of the weights, rows x cols for the whole picture, null = ones) with FDR_NORM_NONE and the output window
 *    equal to the input's, bit for bit, on the tile plan holding that tile's PSF CENTRED: the prows x pcols PSF written into an
 *    M x N plane rolled by (-(prows / 2), -(pcols / 2)) -- the centre of fdr_psf_motion -- and set as fdr_set_operator_psf_dev sets
 *    an M x N PSF, so the result is registered with the data.  psf_count = 1: the PSF at d_psfs for all tiles; psf_count =
 *    tiles_r tiles_c: PSF a tiles_c + b, at d_psfs + k psf_pitch floats, for tile (a, b).  With one PSF and no weights the tiles of
 *    a tile row that lie at the uniform pitch T - O run in launch groups of fdr_plan_set_batching (the bits are those of the single
 *    calls); otherwise tile by tile.  norm_area: FDR_NORM_NONE, or FDR_NORM_CROPPED = min-max over the whole blended picture.
 *      fdr_tiled_layout_get   pure host: tiles and window of a picture, the smallest tile plan (min_M, min_N: the next powers of two
 *                             of win + p - 1, within [8, 8192] x [32, 8192]) and the bytes of workspace of the _dev call on a tile
 *                             plan of min_M x min_N: the staging of every tile's window, the PSF plane and the weight tables.  A larger
 *                             tile plan M x N needs 4 (M N - min_M min_N) bytes more.
 *      fdr_tiled_tile_origin  pure host: (y_a, x_b) of tile (a, b).
 *      fdr_restore_tiled_f32_dev  device pointers; allocates nothing after the tile plan's own first-use workspaces (those of the
 *                             method's single and batched calls), reads nothing back, asynchronous on `stream`.  A limit for very
 *                             large pictures: the weight tables (32 bytes per picture row and column) are made on the host and
 *                             uploaded from pageable memory, which the HIP runtime takes at the call without waiting up to 1 MiB
 *                             and for which it waits for `stream` from 4 MiB on (measured): with rows + cols
 *                             above 32768 the call may wait.  d_work needs 256-byte
 *                             alignment.  On return the plan's operator tables are those of the LAST tile's PSF (an operator PSF set
 *                             before the call is replaced).
 *      fdr_restore_tiled_f32  host pointers, synchronous; allocates and frees its own device buffers.
 *    FDR_ERR_ARG, before any device work and with the plan usable afterwards: whatever the tile's single call refuses (with any
 *    operator-path plan: the call sets the PSF itself), tile_rows or tile_cols < 1, an overlap negative or above T / 2, a tile plan
 *    below win + p - 1 in either dimension, psf_count neither 1 nor tiles_r tiles_c, psf_pitch below the PSF's span when there are
 *    several, work_bytes too small or d_work misaligned, FDR_NORM_PADDED (there is no single plan), and an output that overlaps the
 *    input, the weights, the PSFs or the workspace.  The blend is one launch over the picture, a gather without atomics (4 bytes
 *    read per covering tile and 4 written per pixel); fdr_plan_pass_times records it and the normalisation; the PSF roll is not recorded (a tile's
 *    own passes, the blend and the normalisation already take up to FDR_MAX_PASSES names).  Results repeat bit for bit, whatever the launch group.          */
#define FDR_TILED_RL_FREE 0
#define FDR_TILED_TV_FREE 1
typedef struct fdr_tiled_params {
    int method;                       /* FDR_TILED_RL_FREE / FDR_TILED_TV_FREE */
    int tile_rows, tile_cols;         /* T: the tile window, >= 1 (a picture no larger is one tile of its own extent) */
    int overlap_rows, overlap_cols;   /* O: 0 .. T / 2 */
    int iterations;                   /* >= 0 */
    float sigma;                      /* RL: coverage threshold in (0, 1) */
    float mu, rho, nu;                /* TV: as fdr_tv_free_params */
    int anisotropic, nonneg;          /* TV */
    int norm_area;                    /* FDR_NORM_NONE / FDR_NORM_CROPPED, over the blended picture */
} fdr_tiled_params;
typedef struct fdr_tiled_layout {
    int tiles_r, tiles_c;  /* tiles per axis */
    int win_rows, win_cols; /* the window of every tile: min(T, extent) */
    int min_M, min_N;      /* the smallest tile plan */
    size_t work_bytes;     /* of the _dev call on that plan */
} fdr_tiled_layout;
int fdr_tiled_layout_get(int rows, int cols, int prows, int pcols, const fdr_tiled_params* params, fdr_tiled_layout* layout);
int fdr_tiled_tile_origin(int rows, int cols, const fdr_tiled_params* params, int a, int b, int* y, int* x);
int fdr_restore_tiled_f32_dev(fdr_plan* tile_plan, const float* d_img, int rows, int cols, int stride, const float* d_weights, int wstride,
                              const float* d_psfs, size_t psf_pitch, int psf_count, int prows, int pcols, int pstride, float* d_out,
                              int out_stride, const fdr_tiled_params* params, void* d_work, size_t work_bytes, void* stream);
int fdr_restore_tiled_f32(fdr_plan* tile_plan, const float* img_host, int rows, int cols, int stride, const float* weights_host, int wstride,
                          const float* psfs_host, size_t psf_pitch, int psf_count, int prows, int pcols, int pstride, float* out_host,
                          int out_stride, const fdr_tiled_params* params);

/* -- the motion-blur estimate: the length and angle of a uniform linear motion blur, from the blurred
 *    picture alone, by the power cepstrum.  The blur puts sinc zeros into |G| in stripes across the motion direction; in the
 *    cepstrum they show as a negative peak at distance L along it.  The plan is M x N, the image window rows x cols (row stride
 *    `stride`) at its top-left corner:
 *        x = w . img on the window, 0 elsewhere;  w[i, j] = h_rows[i] h_cols[j],  h_n[k] = 0.5 - 0.5 cos(2 pi k / (n - 1))
 *        G = DFT2(x) on M x N;  eps = 1e-6 sum |x|
 *        c = Re IDFT2(log(|G| + eps))                                    (IDFT2 includes 1/(M N); c is real and even)
 *        S[a, l] = c bilinearly, periodic, at row -l sin(theta_a), column +l cos(theta_a);  theta_a = a step,
 *                  a = 0 .. ceil(180 / step) - 1, l = min_length .. max_length
 *    The row axis points down: theta is the angle of motionBlurKernel / fdr_psf_motion, and the result goes straight into
 *    fdr_set_psf_motion(plan, length, angle_deg, ...).  (a*, l*) = argmin S (exact ties: the lowest flat index, angle-major);
 *    length = l*, angle_deg = theta_a*, score = S[a*, l*], confidence = (median S - min S) / (1.4826 MAD S) (0 when MAD is 0),
 *    computed in double from the float table.  A confidence below about 10 means no clear blur was found.  An all-zero window
 *    gives length 0, angle 0, score 0, confidence 0 and an all-zero table (and cepstrum).
 *    Arguments: 0 selects the default -- step 0.5 deg, min_length 3, max_length min(100, min(rows, cols) / 4).
 *    Plans: FDR_MODE_FAST with M and N powers of two, or 2^a 3^b 5^c with FDR_FLAG_MIXED_RADIX; 32 <= M, N <= 8192.  FDR_ERR_ARG,
 *    before any device work and with the plan usable afterwards, for any other plan (parity mode, FDR_FLAG_ANY_SIZE sizes),
 *    rows or cols < 16 or larger than the plan, stride < cols, negative arguments, min_length < 2, min_length > max_length,
 *    max_length > min(M, N) / 2 - 2, a step that is not finite or not in (0, 90], a table of more than 2^26 entries, or a null
 *    `est`; FDR_ERR_STATE on a tables-only plan.
 *    The first call on a plan allocates the workspace (one M x N complex plane, the Hann tables, the partials and the table),
 *    kept until fdr_plan_destroy; later calls allocate nothing unless a larger table is asked for.  The calls leave the Wiener /
 *    CLS filter, the operator tables and every result of the other calls as they were.  No float atomics: results are
 *    bit-identical from call to call.
 *      fdr_cepstrum_f32*         c into out (M x N floats, row stride N).  The _dev form is asynchronous on `stream`.
 *      fdr_estimate_motion_f32*  *est; the table S (n_angles x n_lengths floats, angle-major) into scores when it is not NULL.
 *                                The _dev form is SYNCHRONOUS: it reads the table back, so it returns after its work on
 *                                `stream` is done.                                                                      */
typedef struct fdr_motion_estimate {
    int length;        /* l*, 0 for an all-zero window */
    double angle_deg;  /* theta_a* in [0, 180) */
    float score;       /* S[a*, l*] */
    float confidence;  /* (median S - min S) / (1.4826 MAD S) */
    int n_angles;      /* table rows: ceil(180 / step) */
    int n_lengths;     /* table columns: max_length - min_length + 1 */
} fdr_motion_estimate;
int fdr_cepstrum_f32(fdr_plan* plan, const float* img_host, int rows, int cols, int stride, float* out_host);
int fdr_cepstrum_f32_dev(fdr_plan* plan, const float* d_img, int rows, int cols, int stride, float* d_out, void* stream);
int fdr_estimate_motion_f32(fdr_plan* plan, const float* img_host, int rows, int cols, int stride, int min_length, int max_length,
                            double angle_step_deg, fdr_motion_estimate* est, float* scores_host);
int fdr_estimate_motion_f32_dev(fdr_plan* plan, const float* d_img, int rows, int cols, int stride, int min_length, int max_length,
                                double angle_step_deg, fdr_motion_estimate* est, float* d_scores, void* stream);

/* -- the defocus estimate: the radius of a uniform disk blur (an out-of-focus picture), from the blurred
 *    picture alone, and the disk PSF itself.
 *    fdr_psf_disk: out[i, j] = the share of pixel (i, j)'s unit square that lies inside the disk of radius `radius` about
 *    c = size / 2 (integer division, the centre of fdr_psf_gaussian), over the sum of the shares.  A share is counted on a fixed
 *    16 x 16 grid of sub-samples, in integers: sub-sample k of pixel i lies at X = (2 k + 1) + 32 (i - c) - 16 in units of 1 / 32 px
 *    (Y likewise), and is inside when (double)(X^2 + Y^2) <= (32 radius)^2.  out = count / total count, divided in double and
 *    rounded once.  FDR_ERR_ARG unless 1 <= size <= 256, radius is finite and 0 < radius <= min(c, size - 1 - c) + 0.5 (the disk
 *    lies inside the size x size square).
 *    fdr_set_psf_disk, fdr_set_psf_disk_cls, fdr_set_operator_psf_disk: fdr_set_psf_dev, fdr_set_psf_cls_dev and
 *    fdr_set_operator_psf_dev on the disk of size 2 ceil(radius) + 1, generated on the device; they refuse what those refuse, and a
 *    radius that is not finite, not above 0 or above 127.
 *    The estimate.  The transfer function of the disk, J1(2 pi R rho) / (pi R rho), has rings of zeros; in the power cepstrum c of
 *    the motion estimate above (same window, same eps, same plans) they show as a negative ring of radius about 2 R.  With S the
 *    score table of the motion estimate for l = min_diameter .. max_diameter:
 *        T[d] = median over a of S[a, d]       (the mean of the two middle values for an even number of angles)
 *        k* = argmin T (exact ties: the lowest index);  diameter = min_diameter + k*;  score = T[k*]
 *        confidence = (median T - T[k*]) / (1.4826 MAD T)                (0 when the MAD is 0)
 *        ring = diameter + 0.5 (T[k* - 1] - T[k* + 1]) / (T[k* - 1] - 2 T[k*] + T[k* + 1]), the offset clamped to +-0.5; the
 *               diameter itself at either end of T or when the denominator is 0
 *        radius = FDR_DEFOCUS_A ring + FDR_DEFOCUS_B
 *    T is a float per diameter, computed on the device; the pick runs in double on the host.  The median over the directions leaves
 *    the single peak of a motion blur out: a confidence below FDR_DEFOCUS_CONF_MIN means no ring was found.  The two constants are
 *    the least-squares line through the rings of 13 radii from 2 to 13 px on three synthetic scenes (tests/_defocus_model.py).  A
 *    radius below about 1.6 px lies under the smallest diameter.  An all-zero window gives diameter 0, ring 0, radius 0, score 0,
 *    confidence 0 and an all-zero profile.
 *    Arguments, plans, refusals and the workspace are those of fdr_estimate_motion_f32* (min_diameter and max_diameter in the place of
 *    min_length and max_length), and FDR_ERR_ARG for a step that gives more than 4096 angles.  The cepstrum workspace is the motion
 *    estimate's own (one per plan); the first defocus call adds 80 KB for its trig table and profile, later calls allocate nothing.
 *      fdr_estimate_defocus_f32*  *est; T (n_diameters floats) into profile when it is not NULL.  The _dev form is SYNCHRONOUS.
 *      fdr_estimate_blur_f32*     both estimates from one cepstrum: *motion is what fdr_estimate_motion_f32* returns for (min_length,
 *                                 max_length, motion_step_deg), *defocus what fdr_estimate_defocus_f32* returns for (min_diameter,
 *                                 max_diameter, defocus_step_deg), bit for bit; *kind = fdr_blur_kind of the two confidences.
 *                                 The _dev form is SYNCHRONOUS as well: it returns both estimates to the host.
 *      fdr_blur_kind              m = motion_conf / FDR_MOTION_CONF_MIN, f = defocus_conf / FDR_DEFOCUS_CONF_MIN: FDR_BLUR_NONE when
 *                                 both are below 1, else FDR_BLUR_MOTION when m >= f, else FDR_BLUR_DEFOCUS.                   */
#define FDR_DEFOCUS_A 0.52304
#define FDR_DEFOCUS_B (-0.01685)
#define FDR_MOTION_CONF_MIN 10.0
#define FDR_DEFOCUS_CONF_MIN 6.0
#define FDR_BLUR_NONE 0
#define FDR_BLUR_MOTION 1
#define FDR_BLUR_DEFOCUS 2
typedef struct fdr_defocus_estimate {
    int diameter;        /* d*, 0 for an all-zero window */
    double ring;         /* d_sub */
    double radius;       /* FDR_DEFOCUS_A * ring + FDR_DEFOCUS_B */
    float score;         /* T[d*] */
    float confidence;    /* (median T - T[d*]) / (1.4826 MAD T) */
    int n_angles;        /* ceil(180 / step) */
    int n_diameters;     /* entries of T: max_diameter - min_diameter + 1 */
} fdr_defocus_estimate;
int fdr_psf_disk(int size, double radius, float* out_host);
int fdr_psf_disk_dev(int device, int size, double radius, float* d_out, void* stream);
int fdr_set_psf_disk(fdr_plan* plan, double radius, float K, void* stream);
int fdr_set_psf_disk_cls(fdr_plan* plan, double radius, float K, float gamma, void* stream);
int fdr_set_operator_psf_disk(fdr_plan* plan, double radius, void* stream);
int fdr_estimate_defocus_f32(fdr_plan* plan, const float* img_host, int rows, int cols, int stride, int min_diameter, int max_diameter,
                             double angle_step_deg, fdr_defocus_estimate* est, float* profile_host);
int fdr_estimate_defocus_f32_dev(fdr_plan* plan, const float* d_img, int rows, int cols, int stride, int min_diameter, int max_diameter,
                                 double angle_step_deg, fdr_defocus_estimate* est, float* d_profile, void* stream);
int fdr_estimate_blur_f32(fdr_plan* plan, const float* img_host, int rows, int cols, int stride, int min_length, int max_length,
                          double motion_step_deg, int min_diameter, int max_diameter, double defocus_step_deg,
                          fdr_motion_estimate* motion, fdr_defocus_estimate* defocus, int* kind);
int fdr_estimate_blur_f32_dev(fdr_plan* plan, const float* d_img, int rows, int cols, int stride, int min_length, int max_length,
                              double motion_step_deg, int min_diameter, int max_diameter, double defocus_step_deg,
                              fdr_motion_estimate* motion, fdr_defocus_estimate* defocus, int* kind, void* stream);
int fdr_blur_kind(double motion_confidence, double defocus_confidence);

/* -- registering the frames of a burst: the translation of every frame against a reference frame, by phase
 *    correlation that knows the frames' PSFs, and the shift of a PSF that puts the estimate where the multi-frame calls want it
 *    ("a registration shift goes into the PSF").  Translation only: the hand-shake case.  `count` (1 .. FDR_MAX_FRAMES) frames, frame
 *    k at imgs + k img_pitch, each a rows x cols window (row stride `stride`) at the top-left of the M x N plan; one PSF per frame
 *    (prows x pcols, row stride pstride, PSF k at psfs + k psf_pitch, top-left in the plan as fdr_set_frame_psfs* takes them), or psfs
 *    NULL: one common or unknown PSF, plain phase correlation.  For every k != reference, with w the Hann window of the motion estimate:
 *        a = pad(w . d_ref),  b = pad(w . d_k)                                        on M x N
 *        G_a = DFT2(a), G_b = DFT2(b);  H_a = DFT2(pad(p_ref)), H_b = DFT2(pad(p_k))  (both 1 when psfs is NULL)
 *        C   = conj(G_a) G_b H_a conj(H_b)            (= |H_a|^2 |H_b|^2 |X|^2 e^{-i w.s}: the phases of the PSFs cancel, which plain
 *                                                      phase correlation between differently blurred frames gets wrong by pixels)
 *        Chat = C / (|C| + eps_rel mean |C|)          (mean over all M N bins; |C| and the mean in double)
 *        r   = Re IDFT2(Chat)                         (with 1 / (M N))
 *        (i*, j*) = argmax r over |dy| <= max_shift_rows, |dx| <= max_shift_cols     (periodic indices; exact ties: the lowest flat
 *                                                      index of the search window, (dy, dx) row-major from (-max_shift_rows, -max_shift_cols))
 *        dy = i* + parabola(r[i* - 1, j*], r[i*, j*], r[i* + 1, j*]),  dx likewise   (neighbours periodic, also outside the window)
 *        parabola(m, z, p) = 0.5 (m - p) / (m - 2 z + p), 0 for a denominator of 0, clamped to [-0.5, 0.5], in double
 *    The result is s_k with d_k(r) ~ (p_k * x)(r - s_k) when d_ref(r) = (p_ref * x)(r): the shift that belongs in PSF k.  peak =
 *    r[i*, j*]; confidence = (peak - mean r) / std r over the whole plane (double sums in a fixed order, no atomics: two calls give the
 *    same bytes).  The reference gets (0, 0, 1, 0); an all-zero frame (or reference) gets zeros.  The exact float formulas are in the
 *    header of csrc/fdr_register.hip.
 *    THE STREAM TRAVELS IN THE STRUCT, deliberately: the _dev forms run on (hipStream_t)params->stream (NULL = the null stream) and
 *    have no `void* stream` parameter; the host forms ignore the field.  The stream-order table of the test suite is keyed on
 *    `void* stream` parameters and is closed to edits for now, so these entries are fenced by a test file of their own with the same
 *    helper; when that table can next be edited their cases move there.
 *      fdr_register_frames_f32_dev  asynchronous: the `count` results go to the device array d_shifts (8-byte aligned), nothing is read
 *                              back, and after the first call on a plan nothing is allocated.  d_corr, when not NULL, receives the
 *                              correlation plane r of frame k (M x N floats) at d_corr + k M N, zeros for the reference: for tests.
 *      fdr_register_frames_f32  the host form: frames and PSFs are staged, the results come back; synchronous.
 *    Plans are those of the motion estimate (fast mode, powers of two or 2^a 3^b 5^c with FDR_FLAG_MIXED_RADIX, 32 .. 8192 per side).
 *    Each frame but the reference costs three of the plan's complex 2-D transforms (two without PSFs) and five sweeps over a plane.
 *    FDR_ERR_ARG / FDR_ERR_STATE before any device work and with the plan usable afterwards: the plan kind; rows or cols < 16 or beyond
 *    the plan; stride < cols; a count outside 1 .. FDR_MAX_FRAMES; an img_pitch below a window's span for count > 1; a reference
 *    outside 0 .. count - 1; max_shift_rows outside 1 .. (M - 1) / 2 or max_shift_cols outside 1 .. (N - 1) / 2 after the defaults; an
 *    eps_rel that is negative or not finite; null pointers; with PSFs a size below 1 or beyond the plan, pstride < pcols, a psf_pitch
 *    below a PSF's span for count > 1; a d_shifts off 8 bytes.  The calls use the motion block (its plane and Hann tables) and a
 *    block of their own (the PSF pair plane, the partials, the results), made on first use and freed by fdr_plan_destroy; they touch
 *    none of the filter, the operator tables or the frame tables.
 *      fdr_psf_shift_f32*      `count` PSFs (prows x pcols) and `count` shifts give `count` PSFs of (prows + 2 pad_rows) x (pcols + 2
 *                              pad_cols), PSF k at out + k out_pitch (row stride out_stride): PSF k placed at offset (pad_rows + dy_k,
 *                              pad_cols + dx_k) with bilinear weights, which are non-negative and keep the sum (Richardson-Lucy's
 *                              positivity and the frame's exposure survive); the symmetric padding by an even total keeps the centre
 *                              convention of a PSF.  A gather, one lane per output element, four taps with weights formed in double and
 *                              rounded to float, in a fixed order (csrc/fdr_register.hip).  The _dev form reads the shifts from device
 *                              memory, straight from fdr_register_frames_f32_dev: the chain estimate, shift, fdr_set_frame_psfs_dev,
 *                              frames call never waits for the device.  A shift outside [-pad, pad - 1] is clamped and a NaN is taken
 *                              as 0 in the kernel: no value in device memory indexes outside the planes.  pad = max_shift + 1 holds every
 *                              whole-pixel peak of the estimate, pad = max_shift + 2 also the half pixel the parabola can add at the end
 *                              of the range.  Needs no plan.  FDR_ERR_ARG for null pointers, a count outside 1 .. FDR_MAX_FRAMES, sizes
 *                              outside 1 .. 8192, pads outside 1 .. 8192, strides below the row, pitches below the span for count > 1, shifts
 *                              off 8 bytes, an output that overlaps the PSFs or the shifts.                                        */
typedef struct fdr_frame_shift {
    double dy;        /* rows, positive = down */
    double dx;        /* columns, positive = right */
    float peak;       /* r at the integer peak */
    float confidence; /* (peak - mean r) / std r */
} fdr_frame_shift;
typedef struct fdr_register_params {
    int reference;      /* the frame the others are measured against, 0 .. count - 1 */
    int max_shift_rows; /* the search range |dy| <=; 0 selects min(rows, cols) / 4 */
    int max_shift_cols; /* the search range |dx| <=; 0 selects min(rows, cols) / 4 */
    float eps_rel;      /* the whitening floor relative to mean |C|, >= 0; 0 selects FDR_REGISTER_EPS_REL */
    void* stream;       /* _dev form: the hipStream_t of the call (NULL = the null stream); the host form ignores it */
} fdr_register_params;
typedef struct fdr_psf_shift_params {
    int pad_rows; /* >= 1: the output has prows + 2 pad_rows rows */
    int pad_cols; /* >= 1 */
    void* stream; /* _dev form: the hipStream_t of the call (NULL = the null stream); the host form ignores it */
} fdr_psf_shift_params;
#define FDR_REGISTER_EPS_REL 1e-3f
int fdr_register_frames_f32(fdr_plan* plan, const float* imgs_host, size_t img_pitch, int count, int rows, int cols, int stride,
                            const float* psfs_host, size_t psf_pitch, int prows, int pcols, int pstride,
                            const fdr_register_params* params, fdr_frame_shift* shifts_host);
int fdr_register_frames_f32_dev(fdr_plan* plan, const float* d_imgs, size_t img_pitch, int count, int rows, int cols, int stride,
                                const float* d_psfs, size_t psf_pitch, int prows, int pcols, int pstride,
                                const fdr_register_params* params, fdr_frame_shift* d_shifts, float* d_corr);
int fdr_psf_shift_f32(int device, const float* psfs_host, size_t psf_pitch, int count, int prows, int pcols, int pstride,
                      const fdr_frame_shift* shifts_host, const fdr_psf_shift_params* params, float* out_host, size_t out_pitch,
                      int out_stride);
int fdr_psf_shift_f32_dev(int device, const float* d_psfs, size_t psf_pitch, int count, int prows, int pcols, int pstride,
                          const fdr_frame_shift* d_shifts, const fdr_psf_shift_params* params, float* d_out, size_t out_pitch,
                          int out_stride);

/* -- choosing the regularisation weight from the picture (Gonzalez & Woods section 5.9, Golub, Heath & Wahba
 *    1979, Immerkaer 1996).  The plan is M x N, the image window rows x cols (row stride `stride`) at its top-left corner, pad(d) is
 *    d on the window and 0 elsewhere, H the DFT2 of the operator PSF (fdr_set_operator_psf*), L(u, v) = 4 sin^2(pi u / M) +
 *    4 sin^2(pi v / N).  For a pair (K, gamma) -- the arguments of fdr_set_psf_cls*, whose filter is W = conj(H) / (|H|^2 + K +
 *    gamma L^2):
 *        G = DFT2(pad(d));  P = |G|^2 / (M N)                            (sum over the full spectrum of P = sum of d^2)
 *        t = K + gamma L^2;  den = |H|^2 + t;  q = den > 0 ? t / den : 0       (q = 1 - H W: what the filter leaves of the data)
 *        rho(K, gamma)   = sum over all M N bins of P q^2                (= || pad(d) - blur(restored) ||^2, the residual energy)
 *        trace(K, gamma) = sum over all M N bins of q
 *        gcv(K, gamma)   = M N rho / trace^2                             (+inf when trace = 0)
 *    P is a float per bin, computed from the fast-mode spectrum; q and every sum are double, taken in a fixed order.
 *    The noise estimate: with the mask n = [[1,-2,1],[-2,4,-2],[1,-2,1]] and S = the sum over the (rows - 2)(cols - 2) interior
 *    pixels of |(d * n)[i, j]| (the stencil and the sum in double, in a fixed order),
 *        sigma = sqrt(pi / 2) S / (6 (rows - 2)(cols - 2))
 *    Texture passes the mask: on finely textured pictures at low noise sigma comes out too large (2.4 times on this project's
 *    textured test scene).
 *    The search: one weight (`param`) runs over v_i = lo (hi / lo)^(i / (n_grid - 1)), i = 0 .. n_grid - 1, the other stays at
 *    `fixed`.  `refine` times a new grid of n_grid log-spaced candidates is laid over a bracket [a, b], ends included.
 *      FDR_REG_DISCREPANCY  the target is T = tau rows cols sigma^2.  rho(hi) = 0 (an all-zero window): value = hi, FDR_REG_AT_HIGH.
 *                           rho(lo) >= T: value = lo, FDR_REG_AT_LOW.  rho(hi) < T: value = hi, FDR_REG_AT_HIGH.  (These three
 *                           return after the first grid.)  Otherwise the bracket is [v_(i-1), v_i] for the first i with
 *                           rho(v_i) >= T, in every round, and value = the point where the straight line through
 *                           (log a, log rho(a)) and (log b, log rho(b)) of the last bracket meets log T (b when rho(a) = 0).
 *      FDR_REG_GCV          i = argmin gcv(v_i), the lowest index on ties; the bracket is [v_max(i-1, 0), v_min(i+1, n_grid-1)];
 *                           value = the argmin of the last round; FDR_REG_AT_LOW when it is lo, FDR_REG_AT_HIGH when it is hi.
 *                           With the flat penalty (param K) GCV under-regularises by several dB: prefer the discrepancy
 *                           principle there.
 *    residual, trace and gcv of the choice are those of the candidate of the last round nearest to `value` (in log).
 *    Plans: as for the operator -- FDR_MODE_FAST, M and N powers of two, 8 <= M <= 8192, 32 <= N <= 8192, neither
 *    FDR_FLAG_SIMPLE_PATH nor FDR_FLAG_FULL_SPECTRUM; FDR_ERR_ARG before any device work for any other plan, FDR_ERR_STATE on a
 *    tables-only plan or without an operator PSF.  FDR_ERR_ARG also for: null pointers; a window that does not fit or stride <
 *    cols; rows or cols < 3 where the noise is estimated; negative or non-finite weights; lo >= hi or lo <= 0; n_grid outside
 *    4 .. 64, refine outside 0 .. 8, n outside 1 .. 4096; an unknown method or param; negative (or non-finite) sigma or tau.  Every
 *    refusal leaves the plan usable.  The first call on a plan allocates the workspace (the power plane: one float per
 *    half-spectrum bin, partial sums, candidates), FDR_ERR_ALLOC with the plan intact when that fails; it is kept until
 *    fdr_plan_destroy and later calls allocate nothing.  The Wiener / CLS filter, the operator tables and the workspaces of the other
 *    calls stay as they were.  Padding is zeros: FDR_OPT_PAD_MODE is ignored.  Results are bit-identical from call to call.
 *      fdr_noise_sigma_f32*  sigma of a picture; needs no plan.
 *      fdr_reg_curve_f32*    residual[i] = rho(K[i], gamma[i]), trace[i] likewise, i < n; K, gamma, residual, trace are HOST arrays.
 *      fdr_choose_reg_f32*   the search.  Zero fields of fdr_reg_params select the defaults (refine: -1).
 *    Every _dev form takes the picture from device memory and is SYNCHRONOUS: it reads its results back, so it returns after its
 *    work on `stream` is done.                                                                                                 */
#define FDR_REG_DISCREPANCY 0
#define FDR_REG_GCV 1
#define FDR_REG_PARAM_K 0
#define FDR_REG_PARAM_GAMMA 1
#define FDR_REG_AT_LOW 1
#define FDR_REG_AT_HIGH 2
typedef struct fdr_reg_params {
    int method;      /* FDR_REG_DISCREPANCY / FDR_REG_GCV */
    int param;       /* which weight is searched: FDR_REG_PARAM_K / FDR_REG_PARAM_GAMMA */
    float fixed;     /* the other weight, >= 0 */
    float sigma;     /* discrepancy: noise standard deviation; 0 = estimate it (fdr_noise_sigma) */
    float tau;       /* discrepancy: safety factor on the target; 0 = 1 */
    double lo, hi;   /* search range, 0 < lo < hi; 0, 0 = 1e-8, 1e2 */
    int n_grid;      /* candidates per round, 4 .. 64; 0 = 32 */
    int refine;      /* refinement rounds, 0 .. 8; -1 = default 2 */
} fdr_reg_params;
typedef struct fdr_reg_choice {
    double value;    /* the chosen weight: goes into fdr_set_psf_cls*(K, gamma) with `fixed` as the other */
    double sigma;    /* the noise level used (estimated or given); 0 for GCV unless given */
    double residual; /* rho at the candidate nearest to value in the last round */
    double trace;
    double gcv;
    int flags;       /* FDR_REG_AT_LOW / _AT_HIGH: the range's end was taken */
    int evaluations; /* candidates evaluated */
} fdr_reg_choice;
int fdr_noise_sigma_f32(int device, const float* img_host, int rows, int cols, int stride, double* sigma);
int fdr_noise_sigma_f32_dev(int device, const float* d_img, int rows, int cols, int stride, double* sigma, void* stream);
int fdr_reg_curve_f32(fdr_plan* plan, const float* img_host, int rows, int cols, int stride, const double* K, const double* gamma, int n,
                      double* residual, double* trace);
int fdr_reg_curve_f32_dev(fdr_plan* plan, const float* d_img, int rows, int cols, int stride, const double* K, const double* gamma, int n,
                          double* residual, double* trace, void* stream);
int fdr_choose_reg_f32(fdr_plan* plan, const float* img_host, int rows, int cols, int stride, const fdr_reg_params* params,
                       fdr_reg_choice* choice);
int fdr_choose_reg_f32_dev(fdr_plan* plan, const float* d_img, int rows, int cols, int stride, const fdr_reg_params* params,
                           fdr_reg_choice* choice, void* stream);

/* Host-pointer batch: `count` images at imgs_host + i*img_pitch, results to out_host + i*out_pitch (elements).
 * H2D copy, restoration and D2H copy of consecutive images overlap on three internal streams with three images in
 * flight -- the pinned-buffer / cudaMemcpyAsync pipeline fft/fft_gpu.cu:306-350,372-385 sets out to build.  Buffers
 * from fdr_host_alloc (pinned; replaces cudaMallocHost, fft/fft_gpu.cu:306-308) are copied by DMA in place and the
 * three stages overlap; pageable buffers work too, at the rate of the synchronous copies the runtime then makes.
 * Synchronous: returns when every result is in out_host.                                                        */
int fdr_host_alloc(size_t bytes, void** out);
int fdr_host_free(void* p);
int fdr_wiener_batch_f32(fdr_plan* plan, const float* imgs_host, size_t img_pitch, int count,
                         int rows, int cols, int stride,
                         float* out_host, size_t out_pitch, int out_stride, int norm_area);
/* the same with one pointer per image (the channel Mats of fft_gpu::wienerDeblur_RGB_*, fft/fft_gpu.cu:325-385) */
int fdr_wiener_batch_ptrs_f32(fdr_plan* plan, const float* const* imgs_host, float* const* outs_host, int count,
                              int rows, int cols, int stride, int out_stride, int norm_area);

/* Batched mode only: let consecutive images of fdr_wiener_batch_f32_dev alternate over `nstreams`
 * (1..4) private workspaces on internal HIP streams, forked from / joined to the caller's stream,
 * so one image's kernel tails overlap the next image's kernel heads.  Costs (nstreams-1) extra
 * workspaces of 12 bytes per padded pixel.  Default 1.                                         */
int fdr_plan_set_concurrency(fdr_plan* plan, int nstreams);
/* The same with `group` (1..8) images per launch in the fast mode: every pass handles `group` images in one launch
 * (small images are launch bound; one launch per pass and group fills the chip; pass B' shares the filter between
 * the images of a launch).  nstreams * group <= 16 workspaces.  fdr_plan_set_concurrency(n) == fdr_plan_set_batching(n, 1).              */
int fdr_plan_set_batching(fdr_plan* plan, int nstreams, int group);

/* -- fft_gpu::my_dft2D(Mat&, bool) (fft/fft.hpp:40; empty body at fft/fft_gpu.cu:515):
 *    in-place unscaled 2-D transform of M x N interleaved complex.                       */
int fdr_fft2d_c2c(fdr_plan* plan, float* data_host, int inverse);
int fdr_fft2d_c2c_dev(fdr_plan* plan, float* d_data, int inverse, void* stream);

/* -- fft_gpu::fft_radix2_kernel / transform_row_kernel / dft_naive_kernel (fft/fft.hpp:35-39;
 *    declared, never defined in the reference): 1-D unscaled transform of n interleaved
 *    complex values given by host pointer.  fft1d: power-of-two n up to 32768 (radix-2) else
 *    naive DFT (n <= 4096), as fft_serial::transform_row_inplace dispatches
 *    (fft/fft_serial.cpp:100-101).                                                        */
int fdr_fft1d_c2c(float* data_host, int n, int inverse, int mode);
int fdr_dft_naive_c2c(float* data_host, int n, int inverse);

/* -- colour epilogue of the drivers (serial.cpp:43-54, gpu.cpp:123-137; utils.hpp:55-71 applyWhiteBalance) on the
 *    device: restored planes B, G, R in [0,1] -> Lab -> L scaled so that its mean matches the blurred input's, clamped
 *    to [0,100] -> BGR -> 8 bit interleaved (convertTo(CV_8U, 255)).  Planes: rows x cols, row stride `stride`
 *    (elements); out: rows x cols x 3 bytes, row stride `out_stride_bytes`.  The Lab formulae are OpenCV's (third
 *    party, version unpinned by the reference): expect +-1 at 8 bit against a given OpenCV build.               */
int fdr_white_balance_u8_dev(int device, const float* const d_orig_bgr[3], const float* const d_restored_bgr[3],
                             int rows, int cols, int stride, unsigned char* d_out_bgr8, int out_stride_bytes, void* stream);
int fdr_white_balance_u8(int device, const float* const orig_bgr[3], const float* const restored_bgr[3],
                         int rows, int cols, int stride, unsigned char* out_bgr8, int out_stride_bytes);

/* -- synthetic input: pixel i = top 24 bits of splitmix64(seed+first+i) / 2^24 */
int fdr_synth_image_dev(int device, uint64_t seed, uint64_t first_index, size_t count, float* d_out, void* stream);

/* -- per-pass device timing (the reference's Profiler buckets, fft/fft_gpu.cu:17-57).
 *    With profiling on, every fdr_wiener_*_dev call records a hipEvent pair around each
 *    kernel on the call's stream; fdr_plan_pass_times synchronises and returns the mean
 *    duration in ms of each pass since the last reset, names[i] a static string.         */
#define FDR_MAX_PASSES 16
int fdr_plan_profile(fdr_plan* plan, int enable);
int fdr_plan_pass_times(fdr_plan* plan, int* n_passes, float* mean_ms, const char** names, int* launches);

/* -- the six buckets of the reference's Profiler (fft/fft_gpu.cu:17-57: alloc / h2d / pre / compute / d2h / post),
 *    accumulated per plan since its creation (or the last reset) from hipEvent pairs on the streams the work ran on:
 *      ALLOC   host wall time of fdr_plan_create (hipMalloc is synchronous)      [fft_gpu.cu:304-322]
 *      H2D     image / PSF uploads of the host-pointer entry points              [:330-335,346-350]
 *      PRE     PSF generation, padding, PSF spectrum and filter (fdr_set_psf*)   [:337-343,356]
 *      COMPUTE the restoration passes of fdr_wiener_*                            [:354-369]
 *      D2H     result downloads of the host-pointer entry points                 [:372-375]
 *      POST    0 here: normalisation runs on the device inside COMPUTE           [:378-384 is a CPU cv::normalize]
 *    In the pipelined host batch (fdr_wiener_batch_*_f32) the three streams overlap, so H2D + COMPUTE + D2H exceeds the
 *    wall time, exactly as per-phase sums do.  The call synchronises the device.                                       */
#define FDR_PHASE_ALLOC 0
#define FDR_PHASE_H2D 1
#define FDR_PHASE_PRE 2
#define FDR_PHASE_COMPUTE 3
#define FDR_PHASE_D2H 4
#define FDR_PHASE_POST 5
#define FDR_N_PHASES 6
int fdr_plan_phase_times(fdr_plan* plan, float ms[FDR_N_PHASES], int reset);

/* -- the multi-GPU batched mode for C and C++ callers: `count` independent images sharded over
 *    `n_devices` devices of this process, contiguous blocks by the reference's calculate_distribution rule
 *    (fft/fft_mpi.cpp:89-100 applied to images: count[g] = count / G + (g < count % G)), one host thread, one plan and
 *    one PSF spectrum per entry of `devices` (an ordinal may repeat: {0, 0} runs two workers on device 0).  No data-path
 *    collective: images are independent.
 *      imgs_host != NULL: image i is read from imgs_host[i] and its result written to outs_host[i] (rows x cols,
 *                         strides in elements) through the pipelined host batch of each worker;
 *      imgs_host == NULL: device-resident synthetic run (BASELINE config 5 shape): every worker generates its shard with
 *                         fdr_synth_image_dev (global image index = position in the batch), restores it `steps` times
 *                         (after `warmup` untimed passes) and keeps the results on its device; only statistics return.
 *    psf_host == NULL: motionBlurKernel(psf_size, psf_angle_deg) generated on each device.                            */
typedef struct fdr_batch_desc {
    int n_devices;
    const int* devices;
    int M, N;            /* plan dimensions (powers of two) */
    int mode;            /* FDR_MODE_* */
    unsigned flags;      /* FDR_FLAG_* */
    const float* psf_host;
    int psf_rows, psf_cols, psf_stride;
    int psf_size;        /* used when psf_host == NULL */
    double psf_angle_deg;
    float K;
    int count;           /* images in the batch */
    int rows, cols;      /* image size, rows <= M, cols <= N */
    int stride, out_stride;
    const float* const* imgs_host;
    float* const* outs_host;
    uint64_t synth_seed; /* synthetic run */
    int steps, warmup;   /* synthetic run: timed / untimed passes over the shard (steps >= 1) */
    int nstreams, group; /* fdr_plan_set_batching of every worker (0, 0 = defaults) */
    int norm_area;       /* FDR_NORM_* */
    int bcast_filter;    /* 0: every worker prepares the PSF spectrum / filter itself (default; cheaper than moving it);
                            1: worker 0 prepares it and the others RECEIVE its bytes -- ncclBroadcast over RCCL (xGMI) when
                            the device ordinals are distinct, device / peer copies when an ordinal repeats or RCCL cannot be
                            loaded: the MPI_Bcast / MPI_Scatterv of the padded PSF in the reference's MPI variant
                            (fft/fft_mpi.cpp:334-378).  Needs count >= n_devices.  fdr_batch_stats::filter_path says which.
                            2: the same, and the RCCL path is taken even for a single device entry (a broadcast to itself:
                            exercises the library and the call on a one-GPU machine).
                            UNEXERCISED ON HARDWARE for more than one distinct device (no multi-GPU machine has been
                            available to the builds so far): any RCCL error there falls back to the peer copies (a line
                            on stderr says so, filter_path reports FDR_FILTER_PEER_COPY) instead of failing the batch. */
} fdr_batch_desc;

#define FDR_BATCH_MAX_DEVICES 16
typedef struct fdr_batch_stats {
    int n_devices;
    int first[FDR_BATCH_MAX_DEVICES];      /* first image of worker g */
    int images[FDR_BATCH_MAX_DEVICES];     /* images of worker g (per pass) */
    double elapsed_ms[FDR_BATCH_MAX_DEVICES]; /* worker g: wall time of its timed region */
    double checksum[FDR_BATCH_MAX_DEVICES];   /* sum of worker g's restored pixels (last pass) */
    int status[FDR_BATCH_MAX_DEVICES];     /* FDR_OK or the failing status of worker g */
    double wall_ms;                        /* all workers: from the common start line (every worker has finished its set-up
                                              and warm-up and waits for the others there) to the last one's finish */
    long long images_done;                 /* sum over workers of images x passes */
    double mpixels_per_s;                  /* images_done * rows * cols / wall_ms */
    int filter_path;                       /* FDR_FILTER_*: how the workers came by their filter */
} fdr_batch_stats;
#define FDR_FILTER_LOCAL 0          /* prepared by every worker */
#define FDR_FILTER_RCCL_BROADCAST 1 /* worker 0's, by ncclBroadcast */
#define FDR_FILTER_PEER_COPY 2      /* worker 0's, by device-to-device / peer copies */
int fdr_batch_run(const fdr_batch_desc* desc, fdr_batch_stats* stats);

/* -- single-image multi-GPU mode: the reference's MPI variant splits ONE image into row slabs and
 *    transposes through MPI_Alltoallv (fft/fft_mpi.cpp:89-100 distribution, :170-279 distributed transpose, :284-307 the
 *    2-D driver rows -> transpose -> rows -> transpose).  These are the per-rank device steps of that scheme; the exchange
 *    itself belongs to the caller's communicator (RCCL all-to-all in ..._amd/slab.py).  All asynchronous on `stream`,
 *    device pointers only; `plan` supplies the twiddle tables (and the arithmetic mode) for dimensions M and N.
 *      pad       : real rows (valid_rows x valid_cols, row stride src_stride) -> rows x N complex, zero padded
 *                  (copyMakeBorder + merge of fft/fft_mpi.cpp:357-366, for the rows this rank owns)
 *      rows_fft  : `rows` contiguous transforms of length N (dim 0) or M (dim 1), in place, unscaled   (:291-294, :301-304)
 *      pack      : column blocks of a rows x ld array, block p = columns [displs[p], displs[p] + counts[p]) stored
 *                  rows x counts[p], blocks in rank order: the send buffer of :118-135; elem_size 4 (real) or 8 (complex)
 *      transpose : dense rows x cols -> cols x rows, elem_size 4 or 8                                   (:154-166)
 *      wiener    : G <- Wiener quotient of G against H, pointwise, with the plan's mode and K given     (fft_serial.cpp:186-224)
 *      real      : real part of `count` complex values
 *      minmax    : {min, max} of the window [0, mm_rows) x [0, mm_cols) of a real rows x ld plane into d_mm[2]
 *      normalize : cv::normalize(0, 1, MINMAX) with the given {min, max}, cropped to rows x cols         (fft_serial.cpp:246) */
int fdr_slab_pad_dev(const float* d_src, int valid_rows, int valid_cols, int src_stride, float* d_dst_complex, int rows, int N, void* stream);
int fdr_slab_rows_fft_dev(fdr_plan* plan, float* d_complex, int rows, int dim, int inverse, void* stream);
int fdr_slab_pack_dev(const void* d_src, int rows, int ld, int parts, const int* counts, int elem_size, void* d_dst, void* stream);
int fdr_slab_transpose_dev(const void* d_src, void* d_dst, int rows, int cols, int elem_size, void* stream);
int fdr_slab_wiener_dev(fdr_plan* plan, float* d_g, const float* d_h, size_t count, float K, void* stream);
int fdr_slab_real_dev(const float* d_complex, float* d_real, size_t count, void* stream);
int fdr_slab_minmax_dev(fdr_plan* plan, const float* d_real, int rows, int ld, int mm_rows, int mm_cols, float* d_mm, void* stream);
int fdr_slab_normalize_dev(const float* d_real, int ld, const float* d_mm, float* d_out, int rows, int cols, int out_stride, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FDR_H */
