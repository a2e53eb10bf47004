/*
 * mifft.h -- C ABI of libmifft, the MI355X (gfx950) batched N-D radix-N FFT.
 *
 * This is the drop-in boundary for the ONE hot path of martinvuyk/hackathon-fft:
 * the GPU overloads of `plan_fft` / `fft` and everything below them.  Every
 * entry point cites the reference interface it replaces (paths relative to the
 * reference repository root).  Plain pointers and sizes only; no torch / HIP
 * types in the signatures (the stream is passed as an opaque `void*` that must
 * be a `hipStream_t`, or NULL for the default stream).
 *
 * The library has NO CPU execution path: every exec entry point runs
 * hand-written HIP kernels on the plan's device and fails with
 * MIFFT_ERR_NO_DEVICE when no gfx950 device is usable.  The CPU restatement of
 * the reference lives in oracle/ and is test infrastructure only.
 *
 * Data layout (reference: fft/fft/fft.mojo:20-46): row-major
 *     x   : (batch, d0[, d1[, ...]], C_in)   C_in  in {1 (real), 2 (re,im)}     (1..MIFFT_MAX_DIMS dims)
 *     out : (batch, d0[, d1[, ...]], 2)      interleaved (re, im)
 * Forward transform is unnormalised with exp(-2*pi*i*nk/N); the inverse uses
 * the conjugate twiddles and scales each transformed dimension by 1/N_dim
 * (fft/fft/_fft.mojo:292-294), i.e. matches numpy.fft.fftn / ifftn over axes
 * 1..ndim.  A real input produces the FULL N-point spectrum
 * (fft/fft/_fft.mojo:254-257), not numpy's half spectrum.  (For real input with 2..4
 * transformed dimensions the last pass may compute only half of the spectrum and store the
 * other half as its conjugate mirror image -- the same values to rounding, exactly Hermitian;
 * never with MIFFT_FLAG_FAITHFUL_STAGES.)  MIFFT_FLAG_HALF_SPECTRUM plans take or give numpy's half spectrum
 * instead (rfftn / irfftn; see the flag below).
 *
 * Environment (read ONCE per process, at the first plan; hackathon_fft_amd/csrc/mifft_config.h):
 *     MIFFT_JIT=0           no runtime specialisation (hipRTC): lengths without a precompiled kernel run
 *                           on the literal-stage kernels instead
 *     MIFFT_JIT_CACHE_DIR   directory of the on-disk cache of runtime-specialised code objects (shared
 *                           between processes / ranks; files are written atomically)
 *     MIFFT_JIT_VERBOSE=1   say on stderr why a runtime specialisation failed
 * Nothing else is configurable in libmifft.so: every size threshold of the plan-time policy is a
 * constant derived from the 256-MiB Infinity Cache (kInfinityCacheBytes).  The measurement switches the
 * scripts under tools/ use (MIFFT_ND_CACHE, MIFFT_NTS_*, MIFFT_FOURSTEP_*, MIFFT_FS_*, MIFFT_ROW2D,
 * MIFFT_JIT_NT, MIFFT_JIT_IMAGE, MIFFT_DPP, MIFFT_HERM*, MIFFT_HS, MIFFT_GRID_PER_CU, MIFFT_ILV) and the fault injection of the tests
 * (MIFFT_TEST_FAIL_SCRATCH_ALLOC) exist only in the LAB build, libmifft_lab.so
 * (-DMIFFT_EXPERIMENTAL -DMIFFT_TESTING, same ABI), together with the experimental kernels that stayed
 * negative results; the host package loads it only when MIFFT_LIBRARY points at it.
 */
#ifndef MIFFT_H
#define MIFFT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIFFT_VERSION_MAJOR 0
#define MIFFT_VERSION_MINOR 1

#define MIFFT_MAX_DIMS 6
#define MIFFT_MAX_STAGES 64

/* element types (in_dtype: any of these; out_dtype: F32 or F64 only,
 * reference: `comptime assert out_dtype.is_floating_point()` fft/fft/_fft.mojo:226) */
typedef enum {
    MIFFT_F32 = 0,
    MIFFT_F64 = 1,
    MIFFT_U8 = 2, /* reference 2-D/3-D tests feed uint8: fft/tests.mojo:467,524 */
    MIFFT_I32 = 3,
    /* the reference casts ANY element type in its first-stage load (`x.load(...).cast[out_dtype]()`,
     * fft/fft/_fft.mojo:243-257); these are widened to the plan's out_dtype in the first pass the same way: */
    MIFFT_I8 = 4,
    MIFFT_I16 = 5,
    MIFFT_U16 = 6,
    MIFFT_F16 = 7,  /* IEEE binary16 */
    MIFFT_BF16 = 8  /* bfloat16: the upper 16 bits of a binary32 */
} mifft_dtype;

/* error codes; the reference raises these as compile-time asserts
 * (fft/fft/fft.mojo:22-46, fft/fft/_utils.mojo:189-220) or DeviceContext errors */
typedef enum {
    MIFFT_OK = 0,
    MIFFT_ERR_BAD_RANK = -1,       /* ndim < 1 or > MIFFT_MAX_DIMS          (fft.mojo:22-26) */
    MIFFT_ERR_BAD_DIM = -2,        /* a transformed dim is < 2              (fft.mojo:43-46) */
    MIFFT_ERR_BAD_COMPONENTS = -3, /* C_in not in {1,2}                     (fft.mojo:30-32) */
    MIFFT_ERR_BAD_DTYPE = -4,      /* out dtype not floating                (_fft.mojo:226)  */
    MIFFT_ERR_BAD_BASES = -5,      /* powers of bases do not multiply to N  (_utils.mojo:206-219) */
    MIFFT_ERR_BASE_ONE = -6,       /* a base equals 1 (or 0)                (_utils.mojo:220) */
    MIFFT_ERR_NO_BASES = -7,       /* empty bases list for a dim            (_utils.mojo:189-191) */
    MIFFT_ERR_BAD_BATCH = -8,      /* batch < 0                                               */
    MIFFT_ERR_TOO_LARGE = -9,      /* a dim does not fit one workgroup's LDS (reference: dims >
                                      max_thread_block_size are unsupported off NVIDIA,
                                      _ndim_fft_gpu.mojo:100-108,514-519)                     */
    MIFFT_ERR_NO_DEVICE = -10,     /* no usable HIP device / device < 0                       */
    MIFFT_ERR_HIP = -11,           /* HIP runtime error; text via mifft_last_error()          */
    MIFFT_ERR_NULL = -12,          /* NULL plan / buffer                                      */
    MIFFT_ERR_ALIAS = -13,         /* x and out overlap (reference is out-of-place)           */
    MIFFT_ERR_BUFFER_TOO_SMALL = -14,
    MIFFT_ERR_UNSUPPORTED = -15    /* a valid request this library does not route (MIFFT_FLAG_HALF_SPECTRUM cases below);
                                      the reason via mifft_last_error(); never silently worked around */
} mifft_status;

/* plan flags */
#define MIFFT_FLAG_NONE 0u
/* Run every user radix stage literally (one LDS pass per stage, one thread per
 * output element, sequential complex-FMA accumulation) exactly as
 * _radix_n_fft_kernel_stockham does (fft/fft/_fft.mojo:189-296).  Default (0)
 * lets the planner fuse consecutive stages into register butterflies when a
 * specialised kernel exists for the dimension.  Mirrors the reference's
 * `_test=` code-path forcing (fft/fft/_ndim_fft_gpu.mojo:453-459). */
#define MIFFT_FLAG_FAITHFUL_STAGES 1u
/* Half-spectrum real transforms (numpy.fft.rfftn / irfftn over axes 1..ndim; no reference counterpart: the reference
 * always produces the full spectrum, fft/fft/_fft.mojo:254-257).  `dims` are the LOGICAL REAL dims d0..d{k-1}; let
 * h = d{k-1} / 2 + 1 and H = d0 * .. * d{k-2} * h.
 *   forward (inverse = 0, in_components = 1, any in_dtype):
 *       x   (batch, d0.., d{k-1}, 1)  ->  out (batch, d0.., h, 2)      = numpy rfftn
 *   inverse (inverse = 1, in_components = 2, in_dtype == out_dtype in {F32, F64}):
 *       x   (batch, d0.., h, 2)       ->  out (batch, d0.., d{k-1}, 1) = numpy irfftn(X, s = dims), 1/N per dimension;
 *       after the other dimensions are inverse-transformed, the imaginary parts of bins 0 and d{k-1} / 2 are ignored
 *       (numpy's handling of an input that is not Hermitian).  x is never written.
 * mifft_plan_in_bytes / out_bytes are those sizes; an inverse plan with ndim >= 2 owns a scratch of H complex per batch
 * entry (mifft_plan_scratch_bytes).  One launch per dimension: the packed real-row kernel of the last dimension (first
 * in a forward plan, last in an inverse one) and an ordinary column pass per other dimension.
 * A wrong in_components for the direction is MIFFT_ERR_BAD_COMPONENTS, a foreign in_dtype of an inverse plan
 * MIFFT_ERR_BAD_DTYPE.  MIFFT_ERR_UNSUPPORTED (with the reason) for:
 *   - an odd last dim, or one below 8;
 *   - MIFFT_FLAG_FAITHFUL_STAGES together with this flag (the reference has no half spectrum to be faithful to);
 *   - a last dim n outside THE LIMITS OF THE PACKED ROWS, the one rule for every mode that runs on these kernels (this flag,
 *     MIFFT_FLAG_DCT and its type 4, the last dim of MIFFT_FLAG_DCT_ND, MIFFT_FLAG_STFT with its spectrogram and MDCT forms,
 *     MIFFT_FLAG_ISTFT with its IMDCT form): n is even, from 8 to 16384; its half n / 2 has no prime factor above 32; and
 *     the row tile -- n / 2 complex elements of the plan's float type per row -- is at most 96 KiB of LDS.  Only a one-row
 *     tile reaches that: F32 rows never do (16384 points are 64 KiB), F64 rows end at 12288 points (exactly 96 KiB; 12320,
 *     the next length with a smooth half, is refused).  From about 10000 points an F64 row keeps its twiddle table in global
 *     memory instead of LDS.  (MIFFT_FLAG_ISTFT alone is narrower in F64, for its carry: see there);
 *   - an outer dim above 4096 points (it would need the four-step routes), or one without a column kernel;
 *   - MIFFT_JIT=0 and a last dim without a precompiled packed-row kernel: precompiled for 128, 480, 1024, 1080 and 1920
 *     points (F32 and F64, input of the plan's own float type); every other length is specialised at run time. */
#define MIFFT_FLAG_HALF_SPECTRUM 2u
/* Transform a subset of the dims (numpy `axes=`, torch `dim=`).  MIFFT_FLAG_KEEP_DIM(d), d in 0 .. MIFFT_MAX_DIMS-1, leaves
 * dim d untransformed: it is carried through like an extra batch dimension.  Layouts, mifft_plan_in_bytes and
 * mifft_plan_out_bytes do not change; an inverse scales by 1/N of the transformed dims only.  `bases_len` still has ndim
 * entries, and a kept dim's entry must be 0.  One launch per transformed dim, innermost first: the first reads x and
 * writes out, the others run in place on out; a pass over dim i runs at stride prod(dims after i) over prod(dims before
 * i) * batch blocks, whether those dims are kept or not.  mifft_plan_stages() is 0 and mifft_plan_kernel_name() "none"
 * for a kept dim; mifft_plan_num_launches() is the number of transformed dims.
 * Refused before any device work:
 *   - a keep bit at d >= ndim, or every dim kept ("no dimension to transform"): MIFFT_ERR_BAD_DIM;
 *   - a nonzero bases_len[d] for a kept dim: MIFFT_ERR_BAD_BASES;
 *   - MIFFT_FLAG_FAITHFUL_STAGES with any keep bit (the reference has no axes to be faithful to): MIFFT_ERR_UNSUPPORTED;
 *   - with MIFFT_FLAG_HALF_SPECTRUM, a kept last dim (numpy halves the last TRANSFORMED axis): MIFFT_ERR_UNSUPPORTED.
 * Routed: the innermost dim transformed up to the single-launch limit of a COMPLEX row (16384 points, F64 8192: 128 KiB; with
 * MIFFT_FLAG_HALF_SPECTRUM the limits of the packed rows above instead); any other transformed dim up to 4096 points.
 * Anything else is MIFFT_ERR_UNSUPPORTED with a reason: masked plans have no four-step, plane, Hermitian or half-store routes.
 * With MIFFT_FLAG_HALF_SPECTRUM the last dim is packed real rows as without a mask and the other transformed dims are
 * column passes over the half-spectrum tensor. */
#define MIFFT_FLAG_KEEP_DIM(d) ((uint32_t)1u << (8 + (d)))
#define MIFFT_FLAG_KEEP_MASK 0x3F00u

/* DCT-II / DCT-III of real rows (scipy.fft.dct / idct of type 2 along the last axis; no reference counterpart).  ndim = 1,
 * dims = {n}, in_components = 1 in both directions; x and out are both REAL, (batch, n, 1):
 *   forward (inverse = 0, any in_dtype):   X[k] = 2 sum_j x[j] cos(pi k (2j+1) / 2n)                = scipy dct(x, 2)
 *   inverse (inverse = 1, in_dtype == out_dtype in {F32, F64}):
 *       x[j] = (X[0] + 2 sum_{k>=1} X[k] cos(pi k (2j+1) / 2n)) / 2n                                = scipy idct(X, 2)
 * With MIFFT_FLAG_DCT_ORTHO (scipy norm="ortho") the forward scales X[0] by sqrt(1/4n) and every other bin by sqrt(1/2n),
 * and the inverse is the transpose of that orthonormal forward; forward then inverse is the identity in both norms.
 * `bases_flat`, when given, lists the radices of the packed N = n / 2-point transform the plan runs and reports: they must
 * multiply to n / 2, not to n (MIFFT_ERR_BAD_BASES otherwise); NULL selects the default estimate for n / 2.
 * x and out need the alignment of one element only (the kernels' wider accesses tolerate any such pointer).
 * mifft_plan_in_bytes / out_bytes are batch * n real elements.  One launch, no scratch: the packed real-row kernel of the
 * N = n / 2-point transform (mifft_plan_stages(0) reports its stages), with the even / odd permutation in its load and the
 * quarter-sample twiddle in its store; mifft_plan_kernel_name(0) is rows<n>[_f64]_dct2_<radices> or ..._dct3_<radices>.
 * in_components != 1 is MIFFT_ERR_BAD_COMPONENTS, a foreign in_dtype of an inverse plan MIFFT_ERR_BAD_DTYPE.
 * MIFFT_ERR_UNSUPPORTED (with the reason), before any device work, for:
 *   - ndim != 1;
 *   - an odd n, or one below 8;
 *   - n outside the limits of the packed rows (MIFFT_FLAG_HALF_SPECTRUM above: n / 2 with a prime factor above 32, n above
 *     16384, a row tile beyond 96 KiB of LDS, which ends F64 rows at 12288 points);
 *   - MIFFT_FLAG_DCT together with MIFFT_FLAG_HALF_SPECTRUM, MIFFT_FLAG_FAITHFUL_STAGES or any keep bit;
 *   - MIFFT_FLAG_DCT_ORTHO without MIFFT_FLAG_DCT or MIFFT_FLAG_DCT_ND;
 *   - MIFFT_JIT=0 and an n without a precompiled instance: precompiled for 1024 points (F32 and F64, input of the plan's
 *     own float type); every other length is specialised at run time. */
#define MIFFT_FLAG_DCT 4u
#define MIFFT_FLAG_DCT_ORTHO 8u
/* DCT-IV of real rows (scipy.fft.dct / idct of type 4; no reference counterpart): a MIFFT_FLAG_DCT plan, with or without
 * MIFFT_FLAG_DCT_ORTHO, whose FIRST `bases` word is the tag MIFFT_DCT_TYPE4_TAG (no radix can equal it: radices multiply to at
 * most 8192).  The optional radices of n / 2 follow the tag; a payload of the tag alone (bases_len[0] = 1) selects the default
 * estimate for n / 2.  Without the tag nothing changes.  x and out are both REAL, (batch, n, 1), in_dtype == out_dtype in
 * {F32, F64} in BOTH directions (MIFFT_ERR_BAD_DTYPE otherwise):
 *   forward:   X[k] = 2 sum_j x[j] cos(pi (2j+1)(2k+1) / 4n)                                            = scipy dct(x, 4)
 *   inverse:   the same sum over X, divided by 2n                                                        = scipy idct(X, 4)
 * With MIFFT_FLAG_DCT_ORTHO both directions scale the sum by sqrt(1 / 2n): the orthonormal DCT-IV, which is its own inverse.
 * One launch, no scratch: a complex row tile of N = n / 2 points (mifft_plan_stages(0) reports its stages) between two
 * twiddles.  With z_m = x[2m] + i x[n-1-2m] and p_m = e^(-i pi (8m+1) / 8n), S = p . FFT_N(p . z) gives X[2k] = 2 Re S_k and
 * X[n-1-2k] = -2 Im S_k; the load forms p . z from two pairs of adjacent reals per work item, the store writes two pairs.  The
 * direction changes only the one scale the store applies: both directions run the same kernel,
 * rows<n>[_f64]_dct4_<radices>_jit, compiled at run time only.  The table p (N complex values, evaluated in long double and
 * rounded once) lives in the plan.  Sizes, slabs, whole_batch, mifft_plan_pass_geometry and the alignment of one element are
 * those of a MIFFT_FLAG_DCT plan, and so is every refusal of one (ndim, odd n, n < 8, the packed configuration of n / 2,
 * the excluded flags, in_components); in addition MIFFT_JIT=0 is MIFFT_ERR_UNSUPPORTED (no precompiled instances), and so is
 * the tag as the first `bases` word of a MIFFT_FLAG_DCT_ND plan (the N-D DCT has no type 4). */
#define MIFFT_DCT_TYPE4_TAG 0x44435434u
/* DST-II / DST-III and DST-IV (scipy.fft.dst / idst / dstn / idstn of types 2 and 4; no reference counterpart): the sine
 * transforms ride on the DCT plans.  No flag and no entry point of their own: the request is a tag as the FIRST `bases` word,
 * as MIFFT_DCT_TYPE4_TAG above (no radix can equal either tag).  With xs[j] = (-1)^j x[j] every DST is its DCT between a sign
 * and an index reversal, DST(x)[k] = DCT(xs)[n-1-k]; both live in the load and the store the DCT tile already has, so the
 * passes, the launch geometry, the tables and the scales are those of the DCT plan of the same shape.
 * MIFFT_DST_TAG ("DST2") on a MIFFT_FLAG_DCT plan, x and out both REAL, (batch, n, 1):
 *   forward (inverse = 0, any in_dtype):   Y[k] = 2 sum_j x[j] sin(pi (k+1)(2j+1) / 2n)             = scipy dst(x, 2)
 *   inverse (inverse = 1, in_dtype == out_dtype in {F32, F64}):
 *       x[j] = ((-1)^j Y[n-1] + 2 sum_{k<n-1} Y[k] sin(pi (k+1)(2j+1) / 2n)) / 2n                   = scipy idst(Y, 2)
 * With MIFFT_FLAG_DCT_ORTHO the forward scales the LAST bin, Y[n-1], by sqrt(1/4n) and every other bin by sqrt(1/2n); the
 * inverse is the transpose of that.  Forward: the permuting load negates the odd samples and the unpacking store writes
 * Y[k-1] = -2 Im(W^k V[k]) and Y[n-1-k] = 2 Re(W^k V[k]), W = e^(-i pi / 2n): four contiguous runs of reals, as the DCT's.
 * Inverse: the four-run load reads bin k of the cosine transform from n-1-k, the store negates the odd samples.  The kernel is
 * rows<n>[_f64]_dst2_<radices>_jit or ..._dst3_<radices>_jit.
 * MIFFT_DST_TAG on a MIFFT_FLAG_DCT_ND plan, as the first word of dimension 0's list (the only word there if dimension 0 is
 * kept): the same transform along EVERY transformed dim (scipy dstn / idstn of type 2).  The last dim runs the row kernel
 * above; another dim the paired-column tile cols<n>[_f64]_dst2_<radices>_jit / ..._dst3_..., whose load gives row j the sign
 * (-1)^j and whose store writes bin k to row n-1-k (forward), or whose load reads bins k and n-k from rows n-1-k and k-1
 * and whose store applies the sign of its row (inverse).  Odd column lengths and every stride of the N-D DCT are served.
 * MIFFT_DST_TYPE4_TAG ("DST4") on a MIFFT_FLAG_DCT plan, in_dtype == out_dtype in {F32, F64} in BOTH directions:
 *   forward:   Y[k] = 2 sum_j x[j] sin(pi (2j+1)(2k+1) / 4n)                                            = scipy dst(x, 4)
 *   inverse:   the same sum over Y, divided by 2n                                                        = scipy idst(Y, 4)
 * With MIFFT_FLAG_DCT_ORTHO both directions scale the sum by sqrt(1 / 2n): the orthonormal DST-IV, its own inverse.  On the
 * DCT-IV tile no address changes: n is even, so the load forms z_m = x[2m] - i x[n-1-2m] and the store writes
 * Y[2k] = -2 Im S_k and Y[n-1-2k] = 2 Re S_k.  The kernel is rows<n>[_f64]_dst4_<radices>_jit in both directions.
 * The optional radices follow the tag in every list as on the DCT plan; a tag alone, and in a tagged payload every empty
 * list of a transformed dim, selects the default estimate.  Without a tag nothing changes.  Sizes, slabs, whole_batch,
 * mifft_plan_pass_geometry, the alignment of one element, the dtype rules and every refusal of the underlying DCT plan are
 * that plan's, with its status codes.  In addition MIFFT_ERR_UNSUPPORTED for:
 *   - MIFFT_JIT=0, for every DST plan: the kernels are compiled at run time only (the precompiled 1024-point DCT rows have no
 *     sine twins);
 *   - MIFFT_DST_TYPE4_TAG on a MIFFT_FLAG_DCT_ND plan (the N-D DST has no type 4).
 * A tag on a plan without MIFFT_FLAG_DCT or MIFFT_FLAG_DCT_ND is an ordinary, and wrong, radix (MIFFT_ERR_BAD_BASES).  Types 1
 * and 3 as scipy's `type` argument, a type 4 over several dims, precompiled instances and sine along one dim with cosine
 * along another in one plan are not provided. */
#define MIFFT_DST_TAG 0x44535432u
#define MIFFT_DST_TYPE4_TAG 0x44535434u
/* N-D DCT-II / DCT-III (scipy.fft.dctn / idctn of type 2 over the transformed dims; no reference counterpart).  ndim = 1 .. 6,
 * in_components = 1 in both directions; x and out are both REAL tensors (batch, d0.., d{k-1}, 1) of one shape.  Every
 * transformed dim gets the 1-D transform of MIFFT_FLAG_DCT above (forward: any in_dtype when the last dim is transformed;
 * inverse: in_dtype == out_dtype in {F32, F64}); MIFFT_FLAG_DCT_ORTHO applies to each of them.  Keep bits
 * (MIFFT_FLAG_KEEP_DIM) mean what they mean elsewhere: a kept dim is carried through like a batch dimension, its
 * mifft_plan_stages() is 0 and its kernel name "none".
 * One launch per transformed dim, innermost first (the 1-D factors of a separable transform commute, so forward and inverse
 * plans run the same order): the first reads x and writes out, the others run in place on out.  No scratch
 * (mifft_plan_scratch_bytes is 0); mifft_plan_in_bytes / out_bytes are batch * d0 * .. * d{k-1} real elements.
 *   - a transformed LAST dim of n points runs the packed-row kernel of MIFFT_FLAG_DCT over the prod / n rows of every
 *     batch entry, with the limits of the packed rows (even, 8 .. 16384, F64 up to 12288, n / 2 without a prime factor above 32);
 *     mifft_plan_stages() reports the stages of its n / 2-point transform, `bases` factor n / 2;
 *     the kernel is rows<n>[_f64]_dct2_<radices> / ..._dct3_<radices>;
 *   - any other transformed dim of n points lies at a stride of S reals (S = the product of the dims after it), S even.  The
 *     same memory viewed as complex elements at stride S / 2 is pairs of adjacent real columns u = x_a + i x_b, which the
 *     in-place column tile moves coalesced.  Forward: the rows are permuted as they are loaded (v[j] = u[2j],
 *     v[n-1-j] = u[2j+1]), Z = FFT_n(v), and with W = e^(-i pi k / 2n) the store separates V_a = (Z[k] + conj Z[n-k]) / 2 and
 *     V_b = (Z[k] - conj Z[n-k]) / 2i and writes row k = (2 Re(W V_a), 2 Re(W V_b)), row n-k = (-2 Im(W V_a), -2 Im(W V_b)).
 *     Inverse: the load forms Z[k] = conj(W) (X[k] - i X[n-k]) / 2 from rows k and n-k (X[n] := 0), the n-point inverse
 *     follows and element j of its result is row 2j (j < ceil(n / 2)), element n-1-j row 2j+1.  F32: every n from 2 to 4096 whose
 *     prime factors are at most 32, odd lengths included.  F64: every such n up to 2056; from 2058 up only the lengths with a
 *     three-pass column configuration (4092 is the longest; 2058, 2080, 2100, 2401, 4000, 4095, 4096 and 150 more are refused:
 *     the radix chooser prefers four passes, whose F64 tile holds at most 4096 elements, and does not retry with three).
 *     mifft_plan_stages() reports n-point stages, `bases` factor n.
 *     The kernel is cols<n>[_f64]_dct2_<radices>_jit / ..._dct3_<radices>_jit: compiled at run time only.
 * mifft_plan_pass_geometry() works for both kinds of pass (a column pass counts tiles of pairs of columns).  Slab execs and
 * whole_batch behave as for every other plan.  x and out need the alignment of one element only.
 * in_components != 1 is MIFFT_ERR_BAD_COMPONENTS, a foreign in_dtype of an inverse plan MIFFT_ERR_BAD_DTYPE.
 * MIFFT_ERR_UNSUPPORTED (with the reason), before any device work, for:
 *   - MIFFT_FLAG_DCT_ND together with MIFFT_FLAG_DCT, MIFFT_FLAG_HALF_SPECTRUM or MIFFT_FLAG_FAITHFUL_STAGES;
 *   - a transformed last dim outside the limits of the packed rows (above), or, under MIFFT_JIT=0, without a precompiled
 *     instance (1024 points);
 *   - a transformed other dim whose stride S is odd;
 *   - a transformed other dim whose stride S is 2 (a trailing extent of 2: a single pair of columns is a row-shaped problem);
 *   - a transformed other dim above 4096 points, one with a prime factor above 32, or one without a fused column configuration
 *     (F64 only: 157 lengths from 2058 up, listed above; "no fused column configuration");
 *   - a forward plan with in_dtype != out_dtype whose last dim is kept (its first pass is a column pass, which reads the
 *     plan's own float type);
 *   - MIFFT_JIT=0 with any transformed dim but the last. */
#define MIFFT_FLAG_DCT_ND 16u
/* Short-time Fourier transform of real signals (torch.stft(..., onesided=True, return_complex=True) with the frames leading; no
 * reference counterpart).  ndim = 2, dims = {T, n}: T samples per batch entry, frames of n samples taken every `hop` samples
 * (MIFFT_FLAG_STFT_HOP(hop), 1 .. 65535).  in_components = 1, inverse = 0, in_dtype == out_dtype in {F32, F64}:
 *       x   (batch, T, 1)  ->  out (batch, F, n / 2 + 1, 2),    out[b, f, k] = sum_j w[j] x~[b, f * hop + j - c] e^(-2 pi i j k / n)
 * with c = 0 and F = 1 + (T - n) / hop without a centre bit (samples after the last frame are never read), c = n / 2 and
 * F = 1 + T / hop with one (integer divisions); x~ is x, continued beyond both ends by reflection without repeating the end
 * samples (MIFFT_FLAG_STFT_CENTER_REFLECT: numpy.pad mode "reflect", torch's pad_mode default) or by zeros
 * (MIFFT_FLAG_STFT_CENTER_ZEROS: torch's pad_mode "constant").  No padded copy of x and no tensor of frames exist: the frames
 * are formed in the load of the one kernel the plan launches, the packed real-row kernel of n points with a framing,
 * windowing load (kernel rows<n>[_f64]_r2c_<radices>_stft_jit: compiled at run time only), which writes the spectrogram once
 * and reads x through the caches, overlapping frames included.
 * `bases_flat` / `bases_len`, when given, have the plan's two entries, and carry the window in the first:
 *   - bases_len[0] is 0 (rectangular window) or 2 n: the IEEE binary64 bits of w[0 .. n-1], each as two 32-bit words, low
 *     word first.  Host data, taken by value: the plan rounds it to its float type and keeps its own device copy;
 *   - bases_len[1] is 0 (the default radix estimate for n: allowed in STFT plans only) or the radices of dim 1, which
 *     multiply to n as those of a half-spectrum plan.
 * NULL / NULL: a rectangular window and the default radices.
 * mifft_plan_stages(0) is 0 and mifft_plan_kernel_name(0) "none" (dim 0 is framed, not transformed); dim 1 reports the n-point
 * stages and the kernel.  mifft_plan_num_launches() is 1, mifft_plan_scratch_bytes() 0, mifft_plan_in_bytes() batch * T
 * elements, mifft_plan_out_bytes() batch * F * (n / 2 + 1) complex; mifft_exec_batch(first, count) offsets x by first * T
 * reals and out by first * F * (n / 2 + 1) complex and touches no other entry; mifft_plan_pass_geometry(1) counts rows of
 * count * F frames; whole_batch behaves as for every other plan.  x needs the alignment of one element only.
 * Refused before any device work, the reason in mifft_last_error().  MIFFT_ERR_UNSUPPORTED:
 *   - a hop field without MIFFT_FLAG_STFT, or the flag with hop 0; a centre bit without the flag, or both centre bits;
 *   - MIFFT_FLAG_STFT with MIFFT_FLAG_FAITHFUL_STAGES, MIFFT_FLAG_HALF_SPECTRUM, MIFFT_FLAG_DCT, MIFFT_FLAG_DCT_ND,
 *     MIFFT_FLAG_DCT_ORTHO or a keep bit;
 *   - ndim != 2;  inverse != 0 (the inverse STFT is not routed through this bit: MIFFT_FLAG_ISTFT, below);
 *   - n outside the limits of the packed rows (MIFFT_FLAG_HALF_SPECTRUM above): odd, below 8, above 16384 (F64: 12288, the
 *     row tile of 96 KiB), n / 2 with a prime factor above 32;
 *   - T < n without a centre bit;  n / 2 > T - 1 with MIFFT_FLAG_STFT_CENTER_REFLECT (one reflection must reach);
 *   - MIFFT_JIT=0 (no precompiled instances).
 * MIFFT_ERR_BAD_DTYPE: in_dtype != out_dtype.  MIFFT_ERR_BAD_COMPONENTS: in_components != 1.  MIFFT_ERR_BAD_BASES: a
 * bases_len[0] other than 0 or 2 n, a window value that is not finite (or radices that do not multiply to n).
 * MIFFT_ERR_TOO_LARGE: T >= 2^31 (or as many frames per entry). */
#define MIFFT_FLAG_STFT 32u
#define MIFFT_FLAG_STFT_CENTER_REFLECT 64u   /* frames centred, signal reflected at both ends */
#define MIFFT_FLAG_STFT_CENTER_ZEROS 128u    /* frames centred, zeros beyond both ends */
#define MIFFT_FLAG_STFT_HOP(h) ((uint32_t)(h) << 16)   /* 1 .. 65535 */
#define MIFFT_FLAG_STFT_HOP_MASK 0xFFFF0000u
/* Inverse short-time Fourier transform with real output (torch.istft(..., onesided=True), the frames leading; no reference
 * counterpart).  Its own mode bit: MIFFT_FLAG_STFT with inverse = 1 stays refused.  It reuses MIFFT_FLAG_STFT_HOP(hop) and
 * the two centre bits -- either one means "centred: the first and last n / 2 samples are trimmed", both together are refused.
 * ndim = 3, dims = {T, F, n}: T output samples per batch entry, F frames (F = 1 is allowed: for this mode only the "no
 * dimension of size 1" rule skips dims[1]) of n points every `hop` samples, 1 <= hop <= n.  inverse = 1, in_components = 2,
 * in_dtype == out_dtype in {F32, F64}:
 *       x (batch, F, n / 2 + 1, 2)  ->  out (batch, T, 1),
 *       out[b, t] = sum_f ws[j] y_f[j] / sum_f w[j]^2,    j = t + c - f * hop,  0 <= j < n,
 * the sums over the frames that cover t; y_f is the n-point inverse real transform (with its 1 / n) of frame f, the imaginary
 * parts of bins 0 and n / 2 ignored as by a half-spectrum inverse; c = n / 2 when centred, else 0; ws = gain * w.
 * With L = n + hop * (F - 1), 2 <= T <= L - c (torch would zero-pad a longer output; this plan refuses it; T = 1 falls to
 * the rule that no dimension but F is of size 1).
 * ONE kernel launch, no scratch, no memset and no tensor of frames: the C2R row kernel of n points over TILE consecutive
 * frames of one entry, whose store overlap-adds the frames in LDS, carries the unfinished samples in LDS to the next tile,
 * divides by the envelope and writes every output sample exactly once with a plain store (kernel
 * rows<n>[_f64]_c2r_<radices>_istft_jit: compiled at run time only).  Every sample is summed in ascending frame order, so the
 * result of an entry is bit-identical for any batch, first / count and grid.
 * `bases_flat` / `bases_len`, when given, have the plan's three entries:
 *   - bases_len[0] is 0 (rectangular window, gain 1), 2 n (the binary64 words of w[0 .. n-1] as in an STFT plan) or 2 n + 2
 *     (w, then one binary64 gain; torch's normalized=True is gain = sqrt(n); the gain does not enter the envelope);
 *   - bases_len[1] is 0;  bases_len[2] is 0 (the default radix estimate for n) or the radices of n.
 * The plan keeps ws[j] / n (rounded once from binary64; the 1 / n is folded into this table, not applied as the pass's scale)
 * and 1 / sum w^2 at all L padded samples as device tables of its float type.
 * mifft_plan_stages / mifft_plan_kernel_name report nothing / "none" for dims 0 and 1 and the n-point stages and the kernel
 * for dim 2; mifft_plan_num_launches() is 1, mifft_plan_scratch_bytes() 0; mifft_plan_in_bytes() / _out_bytes() the two
 * tensors; mifft_exec_batch(first, count) offsets both by whole entries; mifft_plan_pass_geometry(2, count) reports
 * {TILE, threads, n_tiles = count * ceil(F / TILE), grid}: tiles never span entries, and workgroup w of the grid
 * min(CUs * per_cu, max(1, n_tiles / istft_min_run)) (a constant of the library's mifft_config.h) owns the ascending run of tiles from w * len + min(w, rem) on
 * (len = n_tiles / grid, rem = n_tiles % grid; one more tile for w < rem).  whole_batch behaves as for every other plan.
 * Refused before any device work, the reason in mifft_last_error().  MIFFT_ERR_UNSUPPORTED:
 *   - MIFFT_FLAG_ISTFT with MIFFT_FLAG_STFT, MIFFT_FLAG_FAITHFUL_STAGES, MIFFT_FLAG_HALF_SPECTRUM, MIFFT_FLAG_DCT,
 *     MIFFT_FLAG_DCT_ND, MIFFT_FLAG_DCT_ORTHO or a keep bit;  inverse = 0;  ndim != 3;  both centre bits;
 *   - hop 0, or hop > n (gaps between the frames: the envelope would be zero there);
 *   - n outside the limits of the packed rows (as for MIFFT_FLAG_STFT), or a tile and carry beyond the CU's LDS: the carry of
 *     n reals lies beside the row tile, and the two may fill the 160 KiB (the twiddle table moves to global memory first, from
 *     about n = 13300 in F32 and 6650 in F64).  F32 always fits; in F64 tile and carry are n / 2 + n / 2 complex doubles, 160 KiB
 *     exactly at n = 10240, the longest F64 frame (10290, the next length with a smooth half, is refused: the reason names the
 *     "carry");
 *   - a window whose squared overlap-add falls below 1e-11 in absolute value at one of the samples t + c, 0 <= t < T
 *     (torch's own NOLA threshold and range): the reason names the "overlap-add" condition;
 *   - MIFFT_JIT=0 (no precompiled instances).
 * MIFFT_ERR_BAD_DIM: T < 2 or T > L - c.  MIFFT_ERR_TOO_LARGE: L > 2^26 (the envelope table has L entries).
 * MIFFT_ERR_BAD_COMPONENTS: in_components != 2.  MIFFT_ERR_BAD_DTYPE: in_dtype != out_dtype.  MIFFT_ERR_BAD_BASES: a
 * bases_len[0] other than 0, 2 n or 2 n + 2, a non-zero bases_len[1], a window value or gain that is not finite (or radices
 * that do not multiply to n). */
#define MIFFT_FLAG_ISTFT 0x4000u
/* Magnitude, power or filterbanked (mel) spectrogram: a modifier of MIFFT_FLAG_STFT (torch.stft(...).abs().pow(power), then
 * fb.T @ . along the frequencies; no reference counterpart).  dims, hop, centre bits, dtype rules and every refusal of an
 * STFT plan are unchanged; the output is REAL,
 *       x (batch, T, 1)  ->  out (batch, F, n / 2 + 1, 1),    out[b, f, k] = |X[b, f, k]|^power          (M = 0)
 *       x (batch, T, 1)  ->  out (batch, F, M, 1),            out[b, f, m] = sum_k fb[k, m] |X[b, f, k]|^power   (M > 0)
 * with X the bins of the STFT plan above, K = n / 2 + 1.  The modulus (power 1: a correctly rounded sqrt of re^2 + im^2; the
 * squares are not rescaled as hypot would) and the filterbank are folded into the store of the STFT plan's one kernel (kernel
 * rows<n>[_f64]_r2c_<radices>_stft_p<power>[_fb]_jit): the complex spectrogram is never written, no second launch, no scratch.
 * `bases_flat` / `bases_len` must be given, with the plan's two entries:
 *   - bases_len[0] is 2 n + 2 + 2 M K for an integer M >= 0, all values as IEEE binary64 in two 32-bit words, low word first,
 *     in this order: the window w[0 .. n-1] (a rectangular one is written out as ones); one `power`, exactly 1.0 or 2.0; if
 *     M > 0 the filterbank, row-major (K, M) -- the orientation of torchaudio.functional.melscale_fbanks; a librosa-style
 *     (M, K) matrix is transposed by the caller.  Host data, taken by value;
 *   - bases_len[1] as in an STFT plan.
 * The library bands the matrix: of column m it keeps the rows lo = its first non-zero row .. its last non-zero row (zeros in
 * between stay inside the span; a column of zeros keeps nothing and yields an exact 0), the weights rounded once to the plan's
 * float type.  out[b, f, m] is summed over the kept rows in ascending k, one fused multiply-add per term from an exact zero,
 * so a frame's result is bit-identical for any batch, first / count and grid.  The cost of the filterbank is proportional to
 * the sum of the spans: a dense matrix is correct but slow (there is no matrix-core path; a mel filter spans a handful of
 * bins).  Weights may be of either sign.  A log / dB stage and a dense matrix after the bands (MFCC) travel in the tagged
 * payload below; the mel filterbank and the DCT matrix themselves are made by the caller (the Python package has generators).
 * mifft_plan_out_bytes() is batch * F * W elements, W = Q ? Q : (M ? M : K) (Q: the tagged payload, else 0);
 * mifft_exec_batch(first, count) offsets out by first * F * W reals; mifft_plan_pass_geometry(1), mifft_plan_num_launches() (1), mifft_plan_scratch_bytes() (0) and
 * mifft_plan_in_bytes() are the STFT plan's.
 * MIFFT_ERR_UNSUPPORTED, before any device work: the bit without MIFFT_FLAG_STFT (alone, or with MIFFT_FLAG_ISTFT); every
 * refusal of an STFT plan, MIFFT_JIT=0 included.  MIFFT_ERR_BAD_BASES: a bases_len[0] of any other length (the reason names
 * bases_len[0]; NULL bases included: the power has to be given), a power other than 1 or 2 (the reason names the power), a
 * window value, power or filterbank weight that is not finite.  MIFFT_ERR_TOO_LARGE: M > MIFFT_STFT_MAX_BANDS.
 *
 * The tagged payload: two optional stages after the filterbank, in the same launch.  With v the value above (per band, or per
 * bin when M = 0),
 *       y[m] = fma(a, log2(max(v[m] + add, amin)), c)          (log = 1; y = v otherwise)
 *       z[q] = sum_m post[m, q] y[m],  q < Q                   (Q > 0, which needs M > 0)
 * and out is (batch, F, W, 1), W = Q ? Q : (M ? M : K).  log10(max(v, 1e-10)) is a = log10(2), c = 0, add = 0, amin = 1e-10;
 * decibels are a = 10 log10(2); torchaudio's log(v + 1e-6) is add = 1e-6, a = ln 2.  bases_len[0] is then exactly
 * 2 (n + 9 + K M + M Q) words, binary64 values as above, in this order:
 *       w[0 .. n-1] | TAG | power | M | Q | log | add | amin | a | c | fb (K, M) row-major | post (M, Q) row-major
 * TAG is the one NaN with the bits MIFFT_STFT_EXT_TAG_HI : MIFFT_STFT_EXT_TAG_LO, in the slot where the untagged payload has
 * its power (no valid untagged payload has a NaN there; any other NaN is the untagged payload's refusal of its power).  M, Q
 * and log are non-negative integers written as binary64, log 0 or 1; add, amin, a and c are read only when log = 1 and are
 * rounded once to the plan's float type.  The logarithm is the full-precision one, not a native approximation.  post is dense,
 * rounded once to the plan's float type, and z[q] is summed over ascending m, one fused multiply-add per term from an exact
 * zero: a frame's result stays bit-identical for any batch, first / count and grid.  The bands of a frame wait for the matrix
 * in the unused halves of the frame's row in LDS, hence M <= n / 2 - 1 when Q > 0; launches stay 1 and scratch 0 (kernel
 * suffixes _lg and _pm after _fb).  A tagged payload with log = 0 and Q = 0 makes the plan the untagged payload makes.  There
 * is no top_db and no max - 8 clamp (both need the maximum over a whole entry): apply them to the small output.
 * Refusals of a tagged payload, before any device work, each reason naming its field.  MIFFT_ERR_BAD_BASES: bases_len[0] of
 * any other length; M, Q or log not finite, negative or not integral; log above 1; power not 1 or 2; with log = 1 an add that
 * is not finite or is negative, an amin that is not positive or does not round to a normal number of the plan's float type, an
 * a that is not finite or is zero, a c that is not finite; a filterbank or post weight that is not finite.
 * MIFFT_ERR_UNSUPPORTED: Q > 0 with M = 0, or with M > n / 2 - 1.  MIFFT_ERR_TOO_LARGE: M or Q > MIFFT_STFT_MAX_BANDS. */
#define MIFFT_FLAG_STFT_POWER 0x8000u
#define MIFFT_STFT_MAX_BANDS 32768
#define MIFFT_STFT_EXT_TAG_LO 0x46465401u
#define MIFFT_STFT_EXT_TAG_HI 0x7FF84D49u
/* Modified discrete cosine transform (the critically sampled lapped transform of AAC / Vorbis / Opus; no reference
 * counterpart): a MIFFT_FLAG_STFT plan whose window payload carries the tag MIFFT_MDCT_TAG.  M coefficients per frame of 2 M
 * samples, frames every M samples:
 *   flags = MIFFT_FLAG_STFT | MIFFT_FLAG_STFT_CENTER_ZEROS | MIFFT_FLAG_STFT_HOP(M), dims = {T, 2 M}, inverse = 0,
 *   in_components = 1, in_dtype == out_dtype in {F32, F64};
 *       x (batch, T, 1)  ->  out (batch, F, M, 1),    F = (T + M - 1) / M + 1,
 *       out[b, f, k] = scale * sum_{j < 2M} w[j] x~[b, (f - 1) M + j] cos(pi / M (j + 1/2 + M / 2)(k + 1/2)),
 * x~ being x with zeros outside [0, T): every sample lies in two frames, so a window with w[j]^2 + w[j + M]^2 = 1 allows
 * perfect reconstruction (time-domain aliasing cancellation) of all of [0, T).  scale = 1 is the plain MDCT, scale =
 * sqrt(2 / M) the orthonormal DCT-IV of the folded frame.
 *   - bases_len[0] is exactly 2 (2 M) + 4 words: w[0 .. 2M-1] | TAG | scale, binary64 values, low word first; TAG is the one
 *     NaN with the bits MIFFT_MDCT_TAG_HI : MIFFT_MDCT_TAG_LO; scale is finite and not zero.  Host data, taken by value;
 *   - bases_len[1] is 0 (the default estimate) or the radices of M / 2.
 * ONE launch, no scratch, no padded copy and no tensor of frames: the DCT-IV tile above over rows of M reals, whose load
 * frames the signal as the STFT load does, multiplies by the window and folds the 2 M samples y of a frame to M
 * (u[i] = -y[3h-1-i] - y[3h+i], u[h+i] = y[i] - y[M-1-i], i < h = M / 2) as it loads them; out = (scale / 2) DCT-IV(u)
 * (kernel rows<M>[_f64]_dct4_<radices>_mdct_jit, compiled at run time only).  Nothing outside [0, T) of an entry of the exec
 * is read, and a frame's result is bit-identical for any batch, first / count and grid.
 * mifft_plan_out_bytes() is batch * F * M elements; mifft_exec_batch(first, count) offsets x by first * T and out by
 * first * F * M reals; mifft_plan_pass_geometry(1) counts rows of count * F frames; dim 1 reports the stages of M / 2 and the
 * kernel; launches 1, scratch 0.  The STFT's untagged lengths 0 and 2 n keep their meaning, and every other length its refusal.
 * Refused before any device work.  MIFFT_ERR_UNSUPPORTED: a hop other than M; MIFFT_FLAG_STFT_CENTER_REFLECT; no centre bit;
 * MIFFT_FLAG_STFT_POWER; the other flags an STFT plan refuses; ndim != 2; inverse != 0; M outside the limits of a DCT-IV row
 * (the limits of the packed rows: even, 8 .. 16384, F64 up to 12288, M / 2 without a prime factor above 32); MIFFT_JIT=0.
 * MIFFT_ERR_BAD_BASES: a window value or scale that is not finite, a scale of zero (or radices that do not multiply to M / 2).
 * MIFFT_ERR_BAD_DTYPE: in_dtype != out_dtype.  MIFFT_ERR_BAD_COMPONENTS: in_components != 1.  MIFFT_ERR_TOO_LARGE: T >= 2^31.
 * The inverse (IMDCT) is the same tag on a MIFFT_FLAG_ISTFT plan, below. */
#define MIFFT_MDCT_TAG_LO 0x43544401u
#define MIFFT_MDCT_TAG_HI 0x7FF84D44u
/* Inverse MDCT (IMDCT; no reference counterpart): a MIFFT_FLAG_ISTFT plan whose window payload carries the tag MIFFT_MDCT_TAG,
 * mirroring the forward.  F frames of M coefficients per batch entry, overlap-added every M samples:
 *   flags = MIFFT_FLAG_ISTFT | MIFFT_FLAG_STFT_CENTER_ZEROS | MIFFT_FLAG_STFT_HOP(M) (centred: the first M padded samples are
 *   trimmed), ndim = 3, dims = {T, F, 2 M}, inverse = 1, in_components = 1, in_dtype == out_dtype in {F32, F64};
 *       x (batch, F, M, 1)  ->  out (batch, T, 1),    F >= 2,  2 <= T <= (F - 1) M,
 *       y_f[j] = g w[j] sum_{k < M} x[b, f, k] cos(pi / M (j + 1/2 + M / 2)(k + 1/2)),   j < 2 M,
 *       out[b, q M + i] = y_q[M + i] + y_{q+1}[i],     0 <= q <= F - 2,  i < M,  q M + i < T.
 * The first half of frame 0 and the second half of frame F - 1 are never used.  With g = 2 / M (g = sqrt(2 / M) against an
 * MDCT of scale sqrt(2 / M)) and a window with w[j]^2 + w[j + M]^2 = 1 and w[j] = w[2M-1-j] the plan inverts the MDCT plan of
 * the same window (time-domain aliasing cancellation).  There is no envelope to divide by, hence no overlap-add condition.
 *   - bases_len[0] is exactly 2 (2 M) + 4 words: w[0 .. 2M-1] | TAG | g, binary64 values, low word first; g is finite and not
 *     zero.  Host data, taken by value.  A payload of any length whose last four words are TAG | g is this request;
 *   - bases_len[1] is 0;  bases_len[2] is 0 (the default estimate) or the radices of M / 2.
 * Every untagged MIFFT_FLAG_ISTFT payload (0, 2 n, 2 n + 2 words) means what it meant, and every other length keeps its
 * refusal naming bases_len[0].
 * ONE launch, no scratch, no memset, no tensor of frames and no atomics: the DCT-IV tile above over TILE consecutive frames
 * of one entry (kernel rows<M>[_f64]_dct4_<radices>_imdct_jit, compiled at run time only).  Its store finishes the DCT-IV in
 * LDS (v = the plain cosine sums of a frame), reads the unfold y[i] = v[h+i], y[M-1-i] = -v[h+i], y[3h-1-i] = y[3h+i] = -v[i]
 * (i < h = M / 2) straight from the slots of v, and forms every output sample from exactly two products,
 * fma(ws[i], y_{q+1}[i], ws[M+i] y_q[M+i]) with ws = g w rounded once from binary64, the earlier frame first; the pass's
 * own scale is not applied.  The second half of a tile's last frame travels to the workgroup's next tile as h reals in LDS.
 * Workgroups own contiguous ascending runs of tiles exactly as for the inverse STFT (same grid formula); a run that starts
 * inside an entry first transforms ONE frame, the last of the tile before it, with its stores suppressed.  Every sample of
 * [0, T) of every entry of the exec is written exactly once with a plain store, nothing else is written, nothing outside the
 * exec's entries of x is read, and an entry's result is bit-identical for any batch, first / count, whole_batch and grid.
 * mifft_plan_num_launches() is 1, mifft_plan_scratch_bytes() 0; mifft_plan_in_bytes() / _out_bytes() are batch * F * M and
 * batch * T elements; mifft_exec_batch(first, count) offsets x by first * F * M and out by first * T reals;
 * mifft_plan_pass_geometry(2, count) reports {TILE, threads, count * ceil(F / TILE), grid}; dims 0 and 1 report no stages and
 * "none", dim 2 the stages of M / 2 and the kernel.
 * Refused before any device work, the reason in mifft_last_error().  MIFFT_ERR_UNSUPPORTED: a hop other than M; no centre bit,
 * or MIFFT_FLAG_STFT_CENTER_REFLECT; inverse = 0; the other flags an inverse STFT plan refuses; M outside the limits of a
 * DCT-IV row (the limits of the packed rows: even, 8 .. 16384, F64 up to 12288, M / 2 without a prime factor above 32); a tile
 * and carry beyond the CU's LDS (the carry is M / 4 complex elements, half a one-row tile, so tile and carry are at most 144 KiB;
 * the twiddle table moves to global memory first, from about M = 16000 in F32 and 8000 in F64; no admissible M is refused today);
 * MIFFT_JIT=0.  MIFFT_ERR_BAD_DIM: F < 2, T < 2 or T > (F - 1) M.  MIFFT_ERR_BAD_COMPONENTS: in_components != 1.
 * MIFFT_ERR_BAD_DTYPE: in_dtype != out_dtype.  MIFFT_ERR_BAD_BASES: a tagged bases_len[0] other than 2 (2 M) + 4, a non-zero
 * bases_len[1], a window value or g that is not finite, g = 0 (or radices that do not multiply to M / 2).
 * MIFFT_ERR_TOO_LARGE: F > 2^26 or T >= 2^31. */
/* THE ADJOINT OF THE STFT (no reference counterpart): the gradient of a MIFFT_FLAG_STFT plan's result with respect to its
 * signal, as a MIFFT_FLAG_ISTFT plan whose window payload carries the tag MIFFT_STFT_ADJ_TAG.
 *   flags = MIFFT_FLAG_ISTFT | MIFFT_FLAG_STFT_HOP(hop) [| one centre bit, the FORWARD plan's], ndim = 3, dims = {T, F, n} with T
 *   the SIGNAL's length, inverse = 1, in_components = 2, in_dtype == out_dtype in {F32, F64};
 *       x (batch, F, n / 2 + 1, 2)  ->  out (batch, T, 1) [and edge (batch, 2, n / 2)].
 * With c = n / 2 for a centred forward plan (0 otherwise), L = n + hop (F - 1) <= T + 2 c, and g the incoming gradient in the
 * convention dL/dRe X + i dL/dIm X:
 *       p_f[j] = Re sum_{k = 0}^{n / 2} g[b, f, k] exp(+2 pi i j k / n),      j < n,
 *       gxp[b, u] = sum over the frames f that cover u, ascending, of gain w[u - f hop] p_f[u - f hop],   u < L,
 *       out[b, t] = gxp[b, c + t]   for c + t < L;   samples t >= L - c are covered by no frame and NOT written (their
 *       gradient is zero: the caller fills them).
 * MIFFT_FLAG_STFT_CENTER_REFLECT: the padded samples outside the signal are stored too, edge[b, 0, u] = gxp[b, u] for u < c and
 * edge[b, 1, e] = gxp[b, c + T + e] for e < c with c + T + e < L (the rest of side 1 is not written), and the caller folds
 * them back: out[t] += edge[0, c - t] for 1 <= t <= c, out[T - 2 - e] += edge[1, e].  MIFFT_FLAG_STFT_CENTER_ZEROS: they are
 * dropped.  Neither bit: c = 0.
 *   - bases_len[0] is exactly 2 n + 6 words: w[0 .. n-1] | TAG | gain | mode, 0 -- binary64 values, low word first; TAG is the
 *     NaN MIFFT_STFT_ADJ_TAG_HI : MIFFT_STFT_ADJ_TAG_LO; gain, finite and not zero, is a factor on w; mode is one 32-bit word,
 *     the last one reserved, 0.  Host data, taken by value.  Every other MIFFT_FLAG_ISTFT payload length (0, 2 n, 2 n + 2,
 *     the IMDCT's 2 n + 4) means what it meant and keeps its refusals;
 *   - mode 1: x is g.  mode 2: x is X, the forward plan's result, and the exec brings mult = dL/d|X|^2, real,
 *     (batch, F, n / 2 + 1): g = 2 mult X.  mode 3: mult = dL/d|X|: g = mult X / |X|, zero where |X| is.  The product is
 *     formed as the bins are loaded and never written;
 *   - bases_len[1] is 0;  bases_len[2] is 0 (the default estimate) or the radices of n.
 * The exec takes the HOST address of a mifft_stft_adj_args (below) in the place of x:
 *     mifft_stft_adj_args a = { MIFFT_STFT_ADJ_ARGS_MAGIC, x, mult, edge };   mifft_exec_batch(plan, &a, out, first, count, stream);
 * mult is present exactly for modes 2 and 3, edge exactly with MIFFT_FLAG_STFT_CENTER_REFLECT.  Refused with nothing launched:
 * a device address or a block without the magic word, MIFFT_ERR_UNSUPPORTED; x, or a pointer the plan needs, NULL:
 * MIFFT_ERR_NULL; a pointer the plan has no use for: MIFFT_ERR_UNSUPPORTED; x or mult overlapping out or edge, or edge
 * overlapping out, by the sizes of the exec's entries: MIFFT_ERR_ALIAS.  first / count offset all four tensors by whole entries.
 * ONE launch, no scratch, no memset, no atomics: the inverse STFT's tile (kernel rows<n>[_f64]_c2r_<radices>_istft_adj<mode>_jit,
 * compiled at run time only) with bins 0 and n / 2 doubled in the load, the synthesis table gain w / 2 (mode 2: gain w, so its
 * result equals mode 1's on the product 2 mult X bit for bit) and no envelope.  Same runs, warm-up tiles and carry, every
 * sum in ascending frame order: an entry's result is bit-identical for any batch, first / count and grid; every element named
 * above is written exactly once with a plain store and nothing else is.  mifft_plan_num_launches() is 1,
 * mifft_plan_scratch_bytes() 0; mifft_plan_in_bytes() counts x and mult, mifft_plan_out_bytes() out and edge.
 * Refused before any device work, each reason naming the adjoint.  Everything an inverse STFT plan refuses except its covered
 * length (T > L - c), its limit L <= 2^26 and its overlap-add condition -- among them inverse = 0, both centre bits, hop > n,
 * and n beyond the F64 carry limit (10240): MIFFT_ERR_UNSUPPORTED.  MIFFT_ERR_BAD_DIM: L > T + 2 c, or the reflect bit with
 * n / 2 > T - 1.  MIFFT_ERR_BAD_BASES: a mode other than 1, 2, 3, a non-zero reserved word, a gain that is zero or not finite,
 * a window value that is not finite.  MIFFT_ERR_TOO_LARGE: T + n >= 2^31. */
#define MIFFT_STFT_ADJ_TAG_LO 0x4A444101u
#define MIFFT_STFT_ADJ_TAG_HI 0x7FF84D41u
/* the argument block of an STFT adjoint exec (above); the magic word is "MIFFTSA1" */
#define MIFFT_STFT_ADJ_ARGS_MAGIC 0x314153544646494Dull
typedef struct mifft_stft_adj_args {
    uint64_t magic;   /* MIFFT_STFT_ADJ_ARGS_MAGIC */
    const void* x;    /* (batch, F, n / 2 + 1, 2): the gradient (mode 1) or X (modes 2, 3), on the plan's device */
    const void* mult; /* (batch, F, n / 2 + 1) reals of the plan's type, or NULL in mode 1 */
    void* edge;       /* (batch, 2, n / 2) reals of the plan's type, or NULL without MIFFT_FLAG_STFT_CENTER_REFLECT */
} mifft_stft_adj_args;
/* THE ADJOINT OF THE INVERSE STFT (no reference counterpart): the gradient of a MIFFT_FLAG_ISTFT plan's result with respect to
 * its frames, as a MIFFT_FLAG_STFT plan whose window payload carries the tag MIFFT_ISTFT_ADJ_TAG.
 *   flags = MIFFT_FLAG_STFT | MIFFT_FLAG_STFT_HOP(hop) [| MIFFT_FLAG_STFT_CENTER_ZEROS: the inverse plan is centred], ndim = 2,
 *   dims = {T, n} with T the inverse plan's stored samples, inverse = 0, in_components = 1, in_dtype == out_dtype in {F32, F64};
 *       x (batch, T, 1)  ->  out (batch, F, n / 2 + 1, 2),   F from the payload (NOT derived from T: `length` may have cropped).
 * With c = n / 2 for a centred plan (0 otherwise), E[u] = sum_f w[u - f hop]^2 the inverse plan's envelope at padded sample u,
 * gy~ the incoming gradient with zeros outside [0, T), c_0 = c_(n/2) = 1 and every other c_k = 2:
 *       out[b, f, k] = (c_k gain / n) sum_{j < n} w[j] gy~[b, f hop + j - c] / E[f hop + j] exp(-2 pi i j k / n)
 * in the convention dL/dRe X + i dL/dIm X; the imaginary parts of bins 0 and n / 2 are written as exact zeros.
 *   - bases_len[0] is exactly 2 n + 6 words: w[0 .. n-1] | TAG | gain | frames, 0 -- binary64 values, low word first, the window
 *     always written out; TAG is the NaN MIFFT_ISTFT_ADJ_TAG_HI : MIFFT_ISTFT_ADJ_TAG_LO; gain, finite and not zero, is the
 *     inverse plan's; frames is one 32-bit word, F >= 1, the last one reserved, 0.  Host data, taken by value.  Every other
 *     MIFFT_FLAG_STFT payload (0, 2 n, the MDCT's 2 n + 4, those of MIFFT_FLAG_STFT_POWER, the convolutions') means what it meant;
 *   - bases_len[1] is 0 (the default estimate) or the radices of n.
 * Runs through plain mifft_exec_batch(plan, x, out, first, count, stream); no argument block.
 * ONE launch, no scratch, no memset, no atomics: the STFT's tile (kernel rows<n>[_f64]_r2c_<radices>_stft_iadj_jit, compiled at
 * run time only).  Its load multiplies sample t = f hop + j - c by 1 / E[f hop + j] -- the very table the inverse plan divides
 * by, built in binary64 and rounded once -- when 0 <= t < T and SELECTS an exact zero otherwise: neither x nor the table is read
 * there, so x may be followed by anything (NaN included) and a frame that sees no stored sample is an exact zero.  The window
 * table is 2 gain w / n; the store halves bins 0 and n / 2.  A frame's result is bit-identical for any batch, first / count
 * and grid.  mifft_plan_num_launches() is 1, mifft_plan_scratch_bytes() 0.
 * Refused before any device work, each with its own reason: every limit of the inverse plan -- hop > n: MIFFT_ERR_UNSUPPORTED;
 * T < 1 or T > n + hop (F - 1) - c, F < 1: MIFFT_ERR_BAD_DIM (the inverse plan's bound; the Python layer asks 2 <= T of both); F or n + hop (F - 1) beyond 2^26: MIFFT_ERR_TOO_LARGE; an
 * envelope below 1e-11 somewhere in [c, c + T) (the nonzero overlap-add condition): MIFFT_ERR_UNSUPPORTED -- then the STFT
 * tile's (an odd n, n < 8, a frame length it does not plan); MIFFT_FLAG_STFT_CENTER_REFLECT, inverse = 1 and every flag an
 * STFT plan refuses: MIFFT_ERR_UNSUPPORTED; a gain that is zero or not finite, a non-zero reserved word, a window value that
 * is not finite: MIFFT_ERR_BAD_BASES. */
#define MIFFT_ISTFT_ADJ_TAG_LO 0x4A444901u
#define MIFFT_ISTFT_ADJ_TAG_HI 0x7FF84D4Au
/* Fused FFT convolution of real rows (numpy: irfft(rfft(x, n) * G, n)[..., o : o + Lo]; no reference counterpart): a
 * MIFFT_FLAG_STFT plan -- that bit ALONE, no hop, no centre bit -- whose payload starts with the tag MIFFT_CONV_TAG.
 *   flags = MIFFT_FLAG_STFT, ndim = 2, dims = {L, n}, inverse = 0, in_components = 1, in_dtype == out_dtype in {F32, F64};
 *       x (batch, L, 1)  ->  out (batch, Lo, 1),      batch = B * D rows, row r filtered by row r % D of H,
 *       out[r, t] = irfft( rfft(x[r], n) * G[r % D], n )[o + t],   t < Lo,    G = H, or conj(H) with mode bit 0 (correlation).
 * rfft zero-pads the row from sample L to n (L <= n; L may be odd), the inverse's 1 / n is included, and H is the UNNORMALISED
 * rfft of the filter: D rows of n / 2 + 1 complex values of the plan's float type.  n < L + K - 1 gives the circular result.
 * The imaginary parts of the products at bins 0 and n / 2 are ignored, as numpy's irfft ignores them.
 *   - bases_len[0] is exactly 8 words of 32 bits:  TAG_LO | TAG_HI | D | o | Lo | mode | H_LO | H_HI.  The two tag words are
 *     the halves of a NaN that no window value can have (window values are finite), in the place of w[0]; D, o, Lo and mode
 *     are plain unsigned words (mode: bit 0 = correlate, bits 8..15 the storage type of "Half-precision storage" below, every
 *     other bit 0); H_HI : H_LO is the 64-bit DEVICE address of H.
 *     No other payload of a MIFFT_FLAG_STFT plan has length 8 with these first two words; every other payload means what it
 *     meant and keeps its refusals;
 *   - bases_len[1] is 0 (the default estimate) or radices of n, as for an STFT plan.
 * H is the CALLER's buffer, bound when the plan is created: the plan stores the address and never copies or frees it.  It
 * must stay allocated as long as the plan lives; its contents may be rewritten between execs, in stream order with them.
 * ONE launch, no scratch, no padded copy, no spectrum in memory: the packed-row R2C tile of n / 2 complex points with
 * TileCfg::CONV (kernel rows<n>[_f64]_r2c_<radices>_conv_jit, compiled at run time only).  Its load packs and zero-extends
 * the row; after the passes one work item per pair of bins (k, n / 2 - k) unpacks X[k] and X[n/2 - k] in LDS, multiplies them by
 * the two filter bins read from global memory, folds the products back and leaves them where it read them; the same passes
 * run again on the same tables (inverse = conj(F(conj .))), and the store writes only the samples o .. o + Lo - 1, each exactly
 * once, in pairs where the address is aligned to two elements and real by real elsewhere.  Nothing outside the exec's rows
 * is read or written; a row's result is bit-identical for any batch, first / count, whole_batch and grid.
 * mifft_plan_num_launches() is 1, mifft_plan_scratch_bytes() 0; mifft_plan_in_bytes() / _out_bytes() are batch * L and
 * batch * Lo elements; mifft_exec_batch(first, count) offsets x by first * L and out by first * Lo reals and takes the filter
 * row of launch row i as (first + i) % D; mifft_plan_pass_geometry(1, count) counts rows of count; dim 0 reports no stages and
 * "none", dim 1 the stages and the kernel, as an STFT plan.
 * Refused before any device work, the reason in mifft_last_error().  MIFFT_ERR_UNSUPPORTED: n outside the limits of the packed
 * rows (even, 8 .. 16384, F64 up to 12288, n / 2 without a prime factor above 32); L > n; ndim != 2; inverse != 0; a hop, a
 * centre bit, MIFFT_FLAG_STFT_POWER, MIFFT_FLAG_ISTFT, MIFFT_FLAG_FAITHFUL_STAGES, MIFFT_FLAG_HALF_SPECTRUM, MIFFT_FLAG_DCT,
 * MIFFT_FLAG_DCT_ND, MIFFT_FLAG_DCT_ORTHO or a keep bit; MIFFT_JIT=0.  MIFFT_ERR_BAD_BASES: Lo < 1 or o + Lo > n; D < 1; a
 * mode word with a bit other than bit 0 and the storage type in bits 8..15; a null H address or one not aligned to one complex element (or radices that do not
 * multiply to n).  MIFFT_ERR_BAD_BATCH: batch not a multiple of D.  MIFFT_ERR_BAD_DTYPE: in_dtype != out_dtype.
 * MIFFT_ERR_BAD_COMPONENTS: in_components != 1.  MIFFT_ERR_TOO_LARGE: D > 2^30.
 *
 * Overlap-save: the same tag in front of exactly 12 words convolves signal rows of ANY length T (dims = {T, n}; T may exceed
 * n) as F blocks of n samples per row, still in ONE launch with no scratch: x (batch, T, 1) -> out (batch, Lo, 1).
 *     word  0, 1   MIFFT_CONV_TAG_LO, MIFFT_CONV_TAG_HI
 *     word  2      D, the filter rows; signal row r takes filter row r % D
 *     word  3      c, the first sample of every block's circular result that is stored
 *     word  4      S, the samples stored per block, which is also the step between blocks
 *     word  5      mode; bit 0 = correlate (multiply by the conjugate), bits 8..15 the storage type (below), every other bit 0
 *     word  6, 7   H_LO, H_HI: the device address of the filter spectra, D rows of n / 2 + 1 complex values, as above
 *     word  8      F, the blocks per signal row
 *     word  9      s0 as a two's-complement int32: the index in x of block 0's first sample; it may be negative
 *     word 10      Lo, the output samples per signal row
 *     word 11      reserved, 0
 * For signal row r and block f < F:
 *     blk[i] = x[r][s0 + f S + i], 0 <= i < n, zeros outside [0, T) (never loaded);
 *     y = irfft( rfft(blk) * G[r % D], n );
 *     out[r][f S + j] = y[c + j]   for 0 <= j < S and f S + j < Lo.
 * Every output sample is written exactly once, by exactly one block; nothing is added, carried between blocks or zeroed
 * first.  THE CALLER'S CONTRACT: the library does not know the filter length K.  That the stored samples are free of the
 * circular wrap-around -- c >= K - 1 and S <= n - c for a convolution; c = 0 and S <= n - K + 1 for a correlation -- is the
 * caller's business: a payload that breaks it is run as written and returns wrapped samples.  The full linear convolution
 * from sample `a` on is c = K - 1, S = n - K + 1, s0 = a - c, F = ceil(Lo / S) (mf.plan_fftconv(taps=K) derives exactly these).
 * The kernel is the CONV tile with TileCfg::OLS (rows<n>[_f64]_r2c_<radices>_conv_ols_jit, run time only): launch row
 * first * F + i is block i % F of signal i / F, its load starts S samples after the block before it (one pair load where both
 * samples lie inside the row, as aligned as x + s0 + f S happens to be), and its store keeps the S samples from c on.
 * mifft_exec_batch's first / count stay in units of SIGNAL rows: x is offset by first * T, out by first * Lo reals, the launch
 * covers count * F block rows (mifft_plan_pass_geometry counts those), and signal row first + i takes filter row
 * (first + i) % D.  A sample's result depends on its own block alone: bit-identical for any batch, first / count and grid.
 * The 8-word payload means exactly what it meant (L > n and mode = 2 are refused there as before).
 * Refused before any device work: everything above that still applies (flags, inverse, components, dtypes, the limits of n,
 * D, batch % D, mode, H); MIFFT_ERR_BAD_BASES: S < 1 or c + S > n; F < 1 or Lo < 1; Lo outside ((F - 1) S, F S]; s0 <= -n or
 * s0 + (F - 1) S >= T (a block that reads no sample of its row); word 11 non-zero.  MIFFT_ERR_TOO_LARGE: T > 2^30
 * (MIFFT_ERR_BAD_DIM: T < 2).
 *
 * Gates: the same tag in front of exactly 16 words fuses two elementwise gates into either form, still ONE launch, no scratch
 * and no intermediate tensor -- the filter stage of Hyena / H3 / S4 models, y = b . conv(a . x):
 *     xg[r][i] = a[r][i] * x[r][i]                                            (pregate:  a has x's shape and dtype)
 *     out[r][t] = b[r][t] * irfft( rfft(xg[r], n) * G[r % D], n )[o + t]       (postgate: b has out's shape and dtype)
 *     word  0 .. 7  as the 8-word payload: tag, D, o (or c), Lo (or S), mode, H_LO, H_HI
 *     word  8       F.  0: a single block -- words 3 and 4 are o and Lo, words 9 and 10 must be 0, L <= n.
 *                   >= 1: overlap-save -- words 3, 4, 9 and 10 are c, S, s0 and Lo as in the 12-word payload
 *     word  9, 10   s0, Lo (overlap-save)
 *     word 11       gates: bit 0 the pregate, bit 1 the postgate; 1, 2 or 3 (0 and every other bit are refused)
 *     word 12 .. 15 reserved, 0
 * (A skip term d * xg needs no gate: conv(xg, h) + d xg = conv(xg, h') with h'[0] = h[0] + d, which is H + d on every bin of
 * the filter spectrum -- real d, so under the conjugate of a correlation as well.  The caller adds it to H.)
 * The order of operations is part of the contract.  The pregate is ONE multiplication of the loaded sample by its gate, in the
 * plan's float type, before the value reaches LDS; a position the load zero-extends (beyond L; outside [0, T) in
 * overlap-save) reads no gate.  The postgate is ONE multiplication of the finished sample (v * 1/n, signed as in the ungated
 * kernel) by its gate immediately before the store, never folded into the scale.  So the result equals, bit for bit, what
 * the ungated plan of the same shape makes of the rounded products a * x, multiplied by b; gates of ones change nothing.
 * A gate element is addressed by signal row and sample, as x and out are: every output sample is still written exactly once
 * by one block, and a row's result is bit-identical for any batch, first / count, whole_batch and grid.  A gate is read in
 * pairs exactly where x is read, or the result stored, in pairs (an address aligned to ONE element suffices), real by real
 * elsewhere; each element of a gate that belongs to a loaded sample or a stored one is read once, and no other.
 * The kernel is the CONV / OLS tile with TileCfg::GATE = the gates word: rows<n>[_f64]_r2c_<radices>_conv[_ols]_g<1|2|3>_jit, run
 * time only.  The ungated payloads select exactly the kernels they selected.
 * THE EXEC.  Gates are activations -- new tensors on every call -- so they are arguments of the exec, not plan state bound by
 * address as H is.  The exec of a gated plan is mifft_exec / mifft_exec_batch / mifft_time_exec with the HOST address of a
 * mifft_gated_args (below) in the place of x:
 *     mifft_gated_args g = { MIFFT_GATED_ARGS_MAGIC, x, pregate, postgate };   mifft_exec_batch(plan, &g, out, first, count, stream);
 * The block is read before the call returns and may live on the stack.  first / count are signal rows as ever: x and the
 * pregate are offset by first * L (or T) reals, out and the postgate by first * Lo.  A gate pointer is non-null exactly where
 * the plan's bit is set: MIFFT_ERR_NULL for a missing gate (or a null x), MIFFT_ERR_UNSUPPORTED for a gate the plan did not ask
 * for.  A gate may alias x; one that overlaps the exec's part of out is MIFFT_ERR_ALIAS.  A gated plan given the device address
 * of the signal itself, as an ungated plan takes it, or a block without the magic word, is refused with
 * MIFFT_ERR_UNSUPPORTED and a message that names mifft_gated_args; nothing is launched in any of these cases.  (The block
 * travels through the existing entry points: the library's set of exported functions does not change.)
 * mifft_plan_num_launches() is 1, mifft_plan_scratch_bytes() 0; mifft_plan_in_bytes() / _out_bytes() stay the sizes of x and out,
 * which are also the sizes of the pregate and the postgate.
 * Refused before any device work: every check of the 8-word payload (F = 0; L > n among them) or of the 12-word one (F >= 1)
 * with its status; MIFFT_ERR_BAD_BASES: a gates word of 0 or above 3; a non-zero word 12 .. 15; F = 0 with a non-zero word 9
 * or 10.  The tag in front of 13, 14 or 15 words is no convolution payload.  MIFFT_JIT=0 refuses the plan as it does the
 * ungated ones.
 *
 * Partitioned overlap-save: the same tag in front of exactly 20 words, for filters longer than half a block (K > n / 2 + 1,
 * the K = L of Hyena-style models beyond one FFT).  The filter is cut into P partitions of Q taps, k_p = k[p Q .. (p + 1) Q)
 * (the last one zero-filled), and H holds one spectrum per channel and partition: (D, P, n / 2 + 1) complex values,
 * H[d][p] = rfft(k_p of channel d, n).  Output block f of a signal row of T samples is
 *     Y_f = sum over p of rfft(blk_{f,p}, n) * H[d][p],   blk_{f,p}[i] = x[s0 + f S - p Q + i]  (0 <= i < n, zero outside [0, T))
 *     y = irfft(Y_f, n);   out[f S + j] = y[c + j]   for j < S and f S + j < Lo
 * (mode bit 0, correlation: the block starts at s0 + f S + p Q and multiplies by conj(H[d][p])).  A pair (f, p) whose block
 * holds no sample of [0, T) contributes nothing and is neither loaded nor transformed.
 *     word  0 .. 15 as the gated overlap-save payload: tag, D, c, S, mode, H_LO, H_HI, F >= 1, s0, Lo, gates, four zeros --
 *                   except that the gates word 11 may be 0 (no gates: the exec takes the device address of x as ever)
 *     word 16       Q: taps per partition, 1 <= Q <= n - 1
 *     word 17       P: partitions, P >= 1, P Q <= 2^30
 *     word 18, 19   reserved, 0
 * S <= n - Q + 1 (what no wrap-around touches; the caller picks c = Q - 1, s0 = o - c for a convolution, c = 0, s0 = o for a
 * correlation) and c + S <= n.  The overlap-save rule "every block reads a sample of its row" does not apply: a block without
 * a live partition stores zeros; Lo <= 2^30 instead.  Still ONE launch, no scratch, no atomics and no LDS beyond the tile's:
 * TILE launch rows per step of the persistent grid as in overlap-save, the P shifted blocks transformed one after the other
 * in the same LDS tile, the products summed in registers in ascending p -- a fixed order, so a signal row's result is
 * bit-identical for any batch, first / count and grid -- and one inverse per stored block.  The input spectra are recomputed,
 * never stored: the work grows with P (about P / 2 forward transforms per stored block for a causal K = T).  Gates are the
 * 16-word form's, bit for bit (the pregate is read again for every partition); a gated plan takes a mifft_gated_args.
 * The kernel is TileCfg::PART on the OLS tile: rows<n>[_f64]_r2c_<radices>_conv_pols[_g<1|2|3>]_jit, run time only.
 * Refused before any device work, with the statuses of the 12- and 16-word forms: their checks of the flags, n, D, batch % D,
 * mode, H, S, c + S, F and Lo against F and S; MIFFT_ERR_BAD_BASES: Q outside 1 .. n - 1, S > n - Q + 1, P < 1 or
 * P Q > 2^30, Lo > 2^30, a gates word above 3, a non-zero word 12 .. 15, 18 or 19.  The tag in front of 17, 18, 19 or 21
 * words is no convolution payload; the 8-, 12- and 16-word payloads mean what they meant.
 *
 * Half-precision storage: bits 8..15 of the MODE word (word 5) of all four forms -- 8, 12, 16 and 20 words -- and of the
 * MIFFT_CONV_GRAD_TAG form below name the STORAGE type of the rows: 0 the plan's float type (what the word has always
 * meant), MIFFT_F16 (7) or MIFFT_BF16 (8).  Bit 0 stays correlate; every other bit, and every other value in bits 8..15, is
 * MIFFT_ERR_BAD_BASES as before (mode = 2 among them); a storage type on a plan that is not MIFFT_F32 is
 * MIFFT_ERR_BAD_DTYPE.  in_dtype == out_dtype == MIFFT_F32 as ever: the arithmetic, H, the tables and the LDS tile are
 * float.  With a storage type x, both gates and out are arrays of 2-byte elements:
 *   - a load reads a pair of storage elements (4 bytes, aligned to one element) where it read a pair of floats, one element
 *     (2 bytes) at the row ends, and widens each exactly; the pregate is the same single float multiplication of the widened
 *     sample by the widened gate; a position the load zero-extends reads nothing;
 *   - a store computes the finished sample in float exactly as the float plan does (v * 1/n, then the postgate), rounds it
 *     ONCE to the storage type -- to nearest even; MIFFT_F16: overflow gives infinity, subnormals are kept; a NaN stays one
 *     -- and writes a pair where the address is aligned to two storage elements (4 bytes), element by element elsewhere;
 *     every output sample is written exactly once.
 * So the result equals, bit for bit, the F32 plan's on the widened tensors, rounded to nearest even.  What changes besides:
 * the kernel (the float plan's name with `_h16` or `_b16` before `_jit`, e.g. rows16384_r2c_16x8x8x8_conv_ols_g3_b16_jit; run time
 * only, MIFFT_JIT=0 refuses the plan); mifft_plan_in_bytes() / _out_bytes(), which count 2 bytes per element;
 * mifft_exec_batch's offsets, first * L and first * Lo in STORAGE elements for x, out and both gates; the alias checks,
 * which use the storage sizes.  One storage type per plan: x, the gates and out share it. */
#define MIFFT_CONV_TAG_LO 0x4F4E5601u
#define MIFFT_CONV_TAG_HI 0x7FF84D43u
/* the argument block of a gated convolution exec (above); the magic word is "MIFFTGA1" */
#define MIFFT_GATED_ARGS_MAGIC 0x314147544646494Dull
typedef struct mifft_gated_args {
    uint64_t magic;       /* MIFFT_GATED_ARGS_MAGIC */
    const void* x;        /* (batch, L, 1) reals on the plan's device */
    const void* pregate;  /* x's shape and dtype, or NULL where the plan has no pregate */
    const void* postgate; /* out's shape and dtype, or NULL where the plan has no postgate */
} mifft_gated_args;

/*
 * THE FILTER GRADIENT of such a convolution (no reference counterpart): a MIFFT_FLAG_STFT plan -- that bit alone, as above --
 * whose 16-word payload starts with MIFFT_CONV_GRAD_TAG.  dims = {L, n} (overlap-save: {T, n}), batch signal rows as in the
 * forward plan.  With u = the rows the forward plan read (x, or a . x) and gv = the gradient of what it stored (gy, or
 * b . gy), the plan computes
 *     A[p][d][k] = sum over the pairs (row r, block f) of channel d (r % D == d) in slice p of  conj(U[k]) G[k],   0 <= k <= n / 2,
 * U = rfft(u-block, n) of the n samples s0 + f S .. of row r that the forward block loaded (zeros outside the row), G =
 * rfft(g-block, n) of the part of gv the forward block stored, put back where the block had it: g-block[i] =
 * gv[r][f S + i - c] for c <= i < c + S with f S + i - c < Lo, zero elsewhere.  Unscaled; with mode bit 0 (the forward
 * correlated) the conjugate is stored, so that irfft(sum_p A[p][d], n)[0 .. K) is the gradient of filter row d in both
 * cases -- the exact adjoint of the forward blocks, circular where they are -- and its lag 0 the gradient of a skip term.
 *     word  0, 1   MIFFT_CONV_GRAD_TAG_LO, MIFFT_CONV_GRAD_TAG_HI
 *     word  2      D >= 1 filter rows, batch % D == 0
 *     word  3      c: the first stored sample of every block (a single block: the forward plan's o)
 *     word  4      S: the samples stored per block (a single block: Lo), S >= 1, c + S <= n
 *     word  5      mode: bit 0, the forward plan correlated; bits 8..15 the storage type of x and gv (below)
 *     word  6      F >= 1 blocks per row, (F - 1) S < Lo <= F S
 *     word  7      s0: the first sample of block 0 (signed), -n < s0 and s0 + (F - 1) S < L
 *     word  8      Lo >= 1: samples per row of gv
 *     word  9      P: partial sums per channel, 1 <= P <= min(65535, batch / D * F); 0: the library picks it, so that D P
 *                  workgroups fill the device when D alone does not
 *     word 10      stage: 0 the fused gradient described here (every payload written before there were stages); 1, 2 or 3 a
 *                  stage of the FUSED PARTITIONED FILTER GRADIENT below; above 3 reserved, MIFFT_ERR_BAD_BASES
 *     word 11      gates: 0 none (every payload written before there were any), bit 0 the forward plan's pregate, bit 1 its
 *                  postgate (1, 2 or 3); above 3 MIFFT_ERR_BAD_BASES.  See GATES below
 *     word 12 .. 15 reserved, 0
 * A single block is F = 1, s0 = 0, S = Lo, c = o with L <= n; anything else runs the overlap-save geometry (2 <= T <= 2^30).
 * x is (batch, L, 1) real, gv (batch, Lo, 1) real, out (P D, n / 2 + 1, 2), all of the plan's float type (in_dtype ==
 * out_dtype, in_components = 1, inverse = 0).  ONE launch of D P persistent workgroups, no scratch, no atomics: workgroup
 * (d, p) walks a contiguous, ascending slice of the batch / D * F pairs of channel d (lengths differ by one at most), keeps
 * its sums in registers and stores row p D + d once.  x and gv are read once each; the sum of a channel runs in an order
 * the plan fixes (shape and P), so two execs give the same bits.  The kernel is TileCfg::WGRAD on the CONV / OLS tile:
 * rows<n>[_f64]_r2c_<radices>_wgrad[_ols]_jit, run time only (MIFFT_JIT=0 refuses the plan).
 * THE EXEC takes the HOST address of a mifft_conv_grad_args in the place of x, as a gated plan takes its block:
 *     mifft_conv_grad_args g = { MIFFT_CONV_GRAD_ARGS_MAGIC, x, gv };   mifft_exec(plan, &g, out, stream);
 * and covers the whole batch: first != 0 or count != batch is MIFFT_ERR_BAD_BATCH (a slab would be a partial sum).  A
 * device address or a block without the magic word is MIFFT_ERR_UNSUPPORTED, a null member MIFFT_ERR_NULL, x or gv
 * overlapping out MIFFT_ERR_ALIAS; nothing is launched in any of these cases.  mifft_plan_pass_geometry(plan, 1, batch, g)
 * answers {tile (pairs per step), threads, steps of all workgroups, grid = D P}: P is grid / D.  mifft_plan_out_bytes() is
 * the size of the (P D, n / 2 + 1, 2) result.
 * Refused before any device work, with the forward plan's statuses: the flag, direction, dtype and component checks, the
 * limits of n (even, 8 .. 16384, float64 to 12288, n / 2 without a prime factor above 32), D and batch % D; MIFFT_ERR_BAD_BASES for the geometry rules above, a mode word beyond bit 0, P beyond its range, a gates
 * word above 3, a stage word above 3 or a non-zero reserved word.  The 8-, 12- and 16-word MIFFT_CONV_TAG payloads are what they were.
 * Half-precision storage: bits 8..15 of the mode word, as in the MIFFT_CONV_TAG forms above (0, MIFFT_F16 or MIFFT_BF16; an
 * F32 plan only: MIFFT_ERR_BAD_DTYPE otherwise; any other value or bit MIFFT_ERR_BAD_BASES).  x and gv are then arrays of
 * 2-byte elements, widened exactly in both block loads; the sums and the result stay float: mifft_plan_in_bytes() counts 2
 * bytes per element of x, mifft_plan_out_bytes() is unchanged, the alias checks use the storage sizes, and the kernel's name
 * carries `_h16` / `_b16` before `_jit`.  The result equals the F32 plan's on the widened tensors bit for bit.
 * GATES (word 11): the filter gradient of the gated forward plan y = b . conv(a . x) without the products u = a . x and
 * gv = b . gy in memory.  The u-block load multiplies every sample it reads from x by the element of the pregate at the same
 * (row, sample), the g-block load every sample it reads from gy by the element of the postgate at the same (row, t) -- one
 * multiplication of its own in the plan's float type (a storage type is widened first), a position a load zero-extends reads
 * no gate -- so the result equals the ungated plan's on the products a . x and b . gy bit for bit (with a storage type: on the
 * float products of the widened tensors).  The pregate has x's shape and size, the postgate gy's; with a storage type both
 * are 2-byte arrays as x and gy are.  Still one launch, the same grid, no scratch.  The kernel is
 * rows<n>[_f64]_r2c_<radices>_wgrad[_ols]_g<1|2|3>[_h16|_b16]_jit, run time only.
 * THE EXEC of a plan with gates takes the HOST address of a mifft_conv_grad_gated_args, a block with a magic word of its own:
 *     mifft_conv_grad_gated_args g = { MIFFT_CONV_GRAD_GATED_ARGS_MAGIC, x, gy, pregate, postgate };   mifft_exec(plan, &g, out, stream);
 * the whole batch as above.  MIFFT_ERR_UNSUPPORTED with a message that names mifft_conv_grad_gated_args: a
 * mifft_conv_grad_args block, a device address, a block without the magic word; MIFFT_ERR_NULL: a gate the plan has and the
 * block lacks, a null x or gy; MIFFT_ERR_UNSUPPORTED: a gate the plan did not ask for; MIFFT_ERR_ALIAS: x, gy or a gate
 * overlapping out (storage sizes).  Nothing is launched in any of these cases.  The gates may alias x, gy or each other: none
 * is written.  A plan without gates takes the mifft_conv_grad_args block as ever.
 *
 * THE FUSED PARTITIONED FILTER GRADIENT (word 10): the filter gradient of a partitioned convolution (filters longer than half
 * a block, K up to 32 n / 2 taps) as three plans of this tag that transform every block of u and of gv ONCE -- a
 * frequency-domain delay line.  With H = n / 2, Pg = ceil(K / H) lag groups and Fg = ceil(Lo / H) g-blocks:
 *     g-block f holds gv[f H + i], i < H, f H + i < Lo, at index H + i (forward correlated: at index i); zeros elsewhere
 *     u-frame m is the n samples of u from o + m H - H on (forward correlated: from o + m H on), zeros outside [0, L)
 *     A[d][p][k] = sum_b sum_f conj(U[b, d, f - p][k]) G[b, d, f][k]     (forward correlated: U[b, d, f + p], conjugate stored)
 *     gk[d][p H + l] = irfft(A[d][p], n)[l],  l < H
 * It does not depend on how the forward plan chose its Q.  A u-frame that holds no sample of [0, L) is neither transformed nor
 * stored; the live frames are a contiguous range m0 .. m0 + Fu - 1.
 *   stage 1 (MIFFT_CONV_GRAD_STAGE_U): the payload above with c = 0, S = H, F = Fu, s0 = the first sample of u-frame m0, Lo =
 *     Fu H, gates 0 or 1.  The exec reads x (and the pregate) alone -- gy may be NULL -- and STORES rfft of every u-block:
 *     out is (batch, Fu, n / 2 + 1, 2), unscaled, mifft_plan_out_bytes() its size.  P only slices the walk.
 *   stage 2 (MIFFT_CONV_GRAD_STAGE_G): the payload above with c = H (forward correlated: 0), S = H, F = Fg, s0 = 0, Lo,
 *     dims[0] = max(Lo, 2), gates 0 or 2.  The exec reads gy (and the postgate) alone -- x may be NULL -- and stores rfft of
 *     every g-block: out is (batch, Fg, n / 2 + 1, 2).
 *     Both are TileCfg::WSPEC on the WGRAD tile, its two block loads unchanged (zero extension, gates, 16-bit widening):
 *     rows<n>[_f64]_r2c_<radices>_wspecu[_ols][_g1][_h16|_b16]_jit and .._wspecg[_ols][_g2][_h16|_b16]_jit, run time only.
 *     A gates bit the stage does not load is MIFFT_ERR_BAD_BASES.
 *   stage 3 (MIFFT_CONV_GRAD_STAGE_LAGS): the lag-group correlation, a precompiled kernel lag_corr_<f32|f64>_p<2|4|8|16|32>.
 *     dims = {max(Fu, 2), n};  word 3 Fu, word 4 Pg (1 .. 32; above: MIFFT_ERR_UNSUPPORTED), word 5 mode (bit 0 alone),
 *     word 6 Fg, word 7 m0 (signed), word 8 Fg again, word 9 P partial sums per channel (slices of the batch / D entries of a
 *     channel, at most that many and 65535; 0: the library picks 1 unless D ceil((n / 2 + 1) / 256) workgroups leave the
 *     device short), word 11 0.  The exec's block is a mifft_conv_grad_args whose x is U, (batch, Fu, n / 2 + 1, 2), and gy is
 *     G, (batch, Fg, n / 2 + 1, 2), both of the plan's float type; out is (P, D, Pg, n / 2 + 1, 2).  Every sum runs over b
 *     ascending, then f ascending; no atomics: two execs give the same bits.
 * The caller owns U and G (scratch of about four times the bytes of x and gy) and may cut the batch into slabs of whole
 * batch entries, one trio of execs and one partial per slab.
 */
#define MIFFT_CONV_GRAD_STAGE_U 1u
#define MIFFT_CONV_GRAD_STAGE_G 2u
#define MIFFT_CONV_GRAD_STAGE_LAGS 3u
#define MIFFT_CONV_GRAD_TAG_LO 0x44524701u
#define MIFFT_CONV_GRAD_TAG_HI 0x7FF84D47u
/* the argument block of a filter-gradient exec (above); the magic word is "MIFFTWG1" */
#define MIFFT_CONV_GRAD_ARGS_MAGIC 0x314757544646494Dull
typedef struct mifft_conv_grad_args {
    uint64_t magic;  /* MIFFT_CONV_GRAD_ARGS_MAGIC */
    const void* x;   /* (batch, L, 1) reals on the plan's device: what the forward plan read */
    const void* gy;  /* (batch, Lo, 1) reals: the gradient of what it stored */
} mifft_conv_grad_args;
/* the argument block of a GATED filter-gradient exec (word 11 of the payload non-zero); the magic word is "MIFFTWG2" */
#define MIFFT_CONV_GRAD_GATED_ARGS_MAGIC 0x324757544646494Dull
typedef struct mifft_conv_grad_gated_args {
    uint64_t magic;       /* MIFFT_CONV_GRAD_GATED_ARGS_MAGIC */
    const void* x;        /* (batch, L, 1) reals on the plan's device: the forward plan's x, before its pregate */
    const void* gy;       /* (batch, Lo, 1) reals: the gradient of the forward plan's out, before its postgate */
    const void* pregate;  /* x's shape and dtype, or NULL where the plan has no pregate */
    const void* postgate; /* gy's shape and dtype, or NULL where the plan has no postgate */
} mifft_conv_grad_gated_args;

/*
 * TWO-SIGNAL FFT CONVOLUTION / CORRELATION (MIFFT_CONV_PAIR_TAG; no reference counterpart): a MIFFT_FLAG_STFT plan whose 16-word
 * payload starts with MIFFT_CONV_PAIR_TAG.  dims = {L, n}, batch rows, in_components = 1, in_dtype == out_dtype (F32 or F64),
 * inverse = 0.  Both operands are signals: x is (batch, L, 1) real, v (batch, K, 1) real, one row of v per row of x, and out is
 * (batch, Lo, 1) real.  For row r, everything modulo the FFT length n:
 *     xe = zeros(n); xe[ea .. ea + L) = x[r]          ve = zeros(n); ve[eb .. eb + K) = v[r]
 *     y  = irfft(rfft(xe) * G, n),  G = rfft(ve), or conj(rfft(ve)) with mode bit 0 (correlate: y[t] = sum_j ve[j] xe[(t + j) mod n])
 *     out[r, t] = y[o + t],  0 <= t < Lo
 * The imaginary parts of the product at bins 0 and n / 2 are dropped.  n < L + K - 1 gives the circular result.
 *     word  0, 1   MIFFT_CONV_PAIR_TAG_LO, MIFFT_CONV_PAIR_TAG_HI
 *     word  2      K   samples per row of v, K >= 1
 *     word  3      ea  where a row of x starts in its n samples, ea + L <= n
 *     word  4      eb  where a row of v starts in its n samples, eb + K <= n
 *     word  5, 6   o, Lo  the stored samples, Lo >= 1, o + Lo <= n
 *     word  7      mode: bit 0 correlate; every other bit, bits 8..15 included (no 16-bit storage), is refused
 *     word  8..15  0
 * then the radices of n (or none).  scipy.signal.correlate(x, v, "full") is ea = K - 1, eb = 0, o = 0, Lo = L + K - 1 with
 * correlate; fftconvolve(x, v, "full") ea = eb = o = 0, Lo = L + K - 1.  The gradients of a plan are plans of this kind again
 * (INTEGRATION.md).  MIFFT_ERR_BAD_BASES for a value outside these rules or a non-zero reserved word; the flags, dtypes and
 * lengths n the other convolution plans refuse are refused alike (n even, 8 .. 16384, n / 2 without a prime factor above 32;
 * compiled at run time only: MIFFT_JIT=0 is MIFFT_ERR_UNSUPPORTED).  One launch, no scratch; mifft_plan_in_bytes is x's size,
 * mifft_plan_out_bytes out's.  A row's result depends on that row of x and v alone: bit-identical for any batch, slab and grid.
 * THE EXEC takes the HOST address of a mifft_conv_pair_args in the place of x:
 *     mifft_conv_pair_args a = { MIFFT_CONV_PAIR_ARGS_MAGIC, x, v };   mifft_exec(plan, &a, out, stream);
 * mifft_exec_batch(first, count) offsets x by first * L, v by first * K and out by first * Lo samples.  MIFFT_ERR_NULL: x or v
 * NULL; MIFFT_ERR_ALIAS: x or v overlapping the exec's part of out (x == v is allowed: autocorrelation);
 * MIFFT_ERR_UNSUPPORTED: a device address or a block without the magic word.  Nothing is launched in any of these cases.
 */
#define MIFFT_CONV_PAIR_TAG_LO 0x49415001u
#define MIFFT_CONV_PAIR_TAG_HI 0x7FF84D50u
/* the argument block of a two-signal convolution exec (above); the magic word is "MIFFTPA1" */
#define MIFFT_CONV_PAIR_ARGS_MAGIC 0x314150544646494Dull
typedef struct mifft_conv_pair_args {
    uint64_t magic;  /* MIFFT_CONV_PAIR_ARGS_MAGIC */
    const void* x;   /* (batch, L, 1) reals on the plan's device */
    const void* v;   /* (batch, K, 1) reals on the plan's device; may be x itself */
} mifft_conv_pair_args;

typedef struct mifft_plan mifft_plan;

/*
 * mifft_plan_create -- replaces the GPU overload of
 *   plan_fft[in_dtype, out_dtype, in_layout, out_layout, *, bases, inverse,
 *            runtime_twfs, max_cluster_size, _test](*, ctx) -> _GPUPlan
 *   (fft/fft/fft.mojo:161-210; _GPUPlan.__init__ fft/fft/_ndim_fft_gpu.mojo:179-207).
 *
 *  device         HIP device ordinal (>= 0).
 *  ndim, dims     transformed dims d0..d{ndim-1} (the layout minus batch and C).
 *  batch          leading dimension (independent transforms).
 *  in_components  1 = real input, 2 = interleaved complex input.
 *  inverse        0 forward, 1 inverse.
 *  bases_flat / bases_len
 *                 per-dim user radix lists, concatenated; bases_len[d] entries
 *                 belong to dim d.  NULL/NULL selects the reference's GPU default
 *                 (_estimate_best_bases target "gpu", fft/fft/fft.mojo:49-104).
 *                 Lists are normalised exactly like _build_ordered_bases
 *                 (fft/fft/_utils.mojo:162-183).
 *  flags          MIFFT_FLAG_*.
 * The plan owns its device twiddle tables (a few KiB per dimension).  The reference's
 * plan always owns a scratch tensor of the output size (_ndim_fft_gpu.mojo:185); here
 * only three routes do -- query it with mifft_plan_scratch_bytes():
 *   - a STRIDED dimension longer than 4096 points: the two-pass four-step through the scratch
 *     (column tiles of N1 points out -> scratch with a row-granular transposition, column tiles of
 *     N2 points scratch -> out), the default for such dimensions,
 *   - its fallback when a factor has no fused column tile: transpose -> rows -> transpose, and
 *   - a contiguous dimension beyond one LDS row (> 16384 points) whose factorisation
 *     has no transposed-store kernel (the three-launch four-step).
 * Every other plan (all BASELINE configs) works without scratch: the contiguous
 * dimension goes x -> out, the others run in place on out.  Running out of device
 * memory for the scratch is MIFFT_ERR_HIP, never a silent fallback.
 * A strided dimension must span fewer than 2^32 elements (N * stride < 2^32, i.e. one
 * transform below 32 GB): MIFFT_ERR_TOO_LARGE otherwise.
 * mifft_plan_stages() reports the user's literal stages; the executed kernel fuses
 * consecutive stages into 2-4 register-butterfly passes unless
 * MIFFT_FLAG_FAITHFUL_STAGES is set (mifft_plan_kernel_name() shows the fused radices).
 * `runtime_twfs`, `max_cluster_size` have no MI355X meaning and do not exist here.
 */
int mifft_plan_create(mifft_plan** out_plan, int device, int in_dtype, int out_dtype,
                      int ndim, const int64_t* dims, int64_t batch, int in_components,
                      int inverse, const uint32_t* bases_flat, const int32_t* bases_len,
                      uint32_t flags);

/*
 * mifft_plan_create_slab -- mifft_plan_create for ONE SLAB of a batch that is split over several plans (one per GPU,
 * SURVEY.md 8e; the reference has no counterpart: its plan always covers the whole batch, fft/fft/fft.mojo:161-210).
 * `batch` transforms are planned and executed; every choice that depends on the tensor size (streaming / non-temporal
 * twins, cache policy, four-step threshold) is made as for `whole_batch` transforms, so that the slab's results equal
 * the same rows of a single plan over the whole batch BIT FOR BIT.  whole_batch = 0 is mifft_plan_create.
 */
int mifft_plan_create_slab(mifft_plan** out_plan, int device, int in_dtype, int out_dtype,
                           int ndim, const int64_t* dims, int64_t batch, int in_components,
                           int inverse, const uint32_t* bases_flat, const int32_t* bases_len,
                           uint32_t flags, int64_t whole_batch);

/*
 * mifft_exec -- replaces the GPU overload of
 *   fft(output, x, ctx, *, plan)  (fft/fft/fft.mojo:262-323 ->
 *   _run_gpu_nd_fft fft/fft/_ndim_fft_gpu.mojo:462-642).
 * `x` and `out` are DEVICE pointers on the plan's device.  Asynchronous on
 * `stream`; no allocation, no hidden synchronisation (the reference's caller
 * synchronises: fft/bench.mojo:51-52).  `x` is never written; every element of
 * `out` is written; `x` and `out` must not overlap.  One in-flight exec per plan
 * per stream order (same contract as the reference's shared scratch).
 */
int mifft_exec(const mifft_plan* plan, const void* x, void* out, void* stream);

/*
 * mifft_exec_batch -- same as mifft_exec on a sub-range of the leading
 * dimension: transforms `count` batch entries starting at `first` (pointers
 * still address entry 0).  This is what the batch-sharded multi-GPU host uses:
 * every rank runs the same plan on its own contiguous slab.  No reference
 * counterpart (the reference is single-device); the grid-over-batch it
 * generalises is fft/fft/_ndim_fft_gpu.mojo:428-450.
 */
int mifft_exec_batch(const mifft_plan* plan, const void* x, void* out, int64_t first,
                     int64_t count, void* stream);

/* frees device tables; replaces _GPUPlan's destructor (ArcPointer / DeviceBuffer drop) */
void mifft_plan_destroy(mifft_plan* plan);

/* --- plan introspection (the reference exposes these as compile-time values) --- */

/* ordered (descending) per-stage radices of dim `dim` -- _get_ordered_bases_processed_list
 * (fft/fft/_utils.mojo:186-221).  Returns the stage count, or a negative status. */
int mifft_plan_stages(const mifft_plan* plan, int dim, uint32_t* radices_out, int capacity);

/* name of the kernel family chosen for dim `dim` ("generic", "wave1024", ...) */
const char* mifft_plan_kernel_name(const mifft_plan* plan, int dim);

/* tile (transforms per workgroup tile), threads, n_tiles and grid of the launch that an exec of
 * `count` batch entries makes for dimension `dim`; MIFFT_ERR_UNSUPPORTED for a pass that is not one
 * persistent tile_kernel launch, or for a kept dim.  The kernels are persistent: workgroup w walks the
 * tiles w, w + grid, ... (n_tiles > grid: more than one round).  Computed by the launch's own code. */
int mifft_plan_pass_geometry(const mifft_plan* plan, int dim, int64_t count, int64_t geometry_out[4]);

/* number of kernel launches one exec enqueues (reference: d + 2(d-1),
 * fft/fft/_ndim_fft_gpu.mojo:634-642) */
int mifft_plan_num_launches(const mifft_plan* plan);

/* required sizes in bytes of x and out for the full batch */
size_t mifft_plan_in_bytes(const mifft_plan* plan);
size_t mifft_plan_out_bytes(const mifft_plan* plan);
/* bytes of the plan-owned scratch tensor (0 for plans that need none, see mifft_plan_create);
 * reference: _GPUPlan.calc_buf, fft/fft/_ndim_fft_gpu.mojo:176-185, which exists for every plan */
size_t mifft_plan_scratch_bytes(const mifft_plan* plan);

/*
 * mifft_plan_device_status -- device-side error flags of the execs enqueued so far with this plan on `stream`;
 * reads and clears them.  Only the experimental L2-resident image kernel of the LAB build can raise one: its
 * XCD-local barrier spins are bounded, and an exec whose spin expired (bit 0) or that was dispatched with a surplus
 * workgroup on one XCD (bit 1) has produced output that must not be trusted.  Every other kernel family has no
 * inter-workgroup dependency and reports 0 without touching the device.  SYNCHRONISES `stream` when the plan
 * contains such a pass -- this is a check to run after a batch of execs, not part of the exec path.
 * No reference counterpart (the reference's only device-wide synchronisation is the kernel boundary,
 * fft/fft/_ndim_fft_gpu.mojo:634-642).
 */
int mifft_plan_device_status(const mifft_plan* plan, void* stream, uint32_t* flags_out);

/* --- planner helpers, usable without a device (pure host logic) --- */

/* _build_ordered_bases (fft/fft/_utils.mojo:162-183) + the product / base==1 checks of
 * _get_ordered_bases_processed_list (:186-221).  Returns stage count or negative status. */
int mifft_ordered_bases(uint32_t length, const uint32_t* bases, int nbases,
                        uint32_t* ordered_out, int capacity);

/* _estimate_best_bases (fft/fft/fft.mojo:49-104); target_gpu != 0 selects the "gpu"
 * branch (:61-80), else the prime list (:83-104).  Returns count or negative status. */
int mifft_estimate_bases(uint32_t length, int target_gpu, uint32_t* bases_out, int capacity);

/* --- diagnostics --- */
const char* mifft_last_error(void);       /* thread-local text of the last failure */
const char* mifft_status_string(int status);
int mifft_version(void);                  /* major*100 + minor */
int mifft_device_count(void);             /* usable HIP devices, 0 if none */

/*
 * mifft_time_exec -- enqueue `iters` back-to-back mifft_exec calls on `stream`
 * bracketed by HIP events recorded on that same stream and return the average
 * milliseconds per exec in *ms_out (synchronises the events, not the device).
 * Measurement helper for bench.py's roofline line; mirrors the timed loop of
 * fft/bench.mojo:48-54.
 */
int mifft_time_exec(const mifft_plan* plan, const void* x, void* out, void* stream, int iters,
                    float* ms_out);

/*
 * mifft_jit_precompile -- build (do not load) the runtime-specialised fused kernel that plan creation would use for
 * a dimension of `length` points without a precompiled table entry, and report the size of its gfx950 code object.
 * The reference compiles every shape at build time (shapes are Mojo comptime parameters, fft/fft/fft.mojo:123-135);
 * libmifft specialises its tile kernel with hipRTC on first use and caches the result per process.  Needs no
 * device: usable to warm the cache ahead of plan creation or to check a length on a build machine.
 * in_dtype: element type of the tensor the pass reads (any mifft_dtype; widened to out_dtype in the load);
 * out_dtype: MIFFT_F32 / MIFFT_F64; strided: 0 contiguous rows, 1 the in-place column-tile form, 2 a fused
 * length x length plane (two innermost dimensions in one LDS tile), k >= 8 a fused k x length plane (length = the
 * contiguous side); real_input != 0: the C_in = 1 twin.
 * Returns MIFFT_OK, or MIFFT_ERR_TOO_LARGE when the length has no fused configuration (a prime factor above 4093,
 * three prime factors above 31, or a tile beyond the 160 KiB of LDS) -- such lengths run on the literal-stage kernels.
 */
int mifft_jit_precompile(int in_dtype, int out_dtype, int64_t length, int strided, int real_input,
                         size_t* code_bytes_out);

#ifdef __cplusplus
}
#endif
#endif /* MIFFT_H */
