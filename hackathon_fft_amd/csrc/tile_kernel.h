// tile_kernel.h -- register-butterfly Stockham tile kernel template for MI355X (gfx950).
//
// One kernel per dimension.  A workgroup owns a TILE of independent transforms of one
// dimension; the tile lives in LDS for the whole transform and HBM is touched exactly once
// for reading and once for writing:
//
//   pass 0      : work item = one radix-R0 butterfly; its R0 inputs come straight from HBM
//                 (lanes -> consecutive elements, so every wave instruction reads whole
//                 contiguous runs), DFT_R0 in registers, results scattered into LDS at the
//                 Stockham-permuted positions        dst[q*P*R + s*P + p]
//   pass 1..k-2 : LDS -> registers (stride N/R gather, conflict-free), twiddle W_{P R}^{j p},
//                 DFT_R in registers, registers -> LDS (same buffer, after a barrier)
//   pass k-1    : as above, but the results go straight to HBM in natural order
//                 (for the last stage q = 0, so lanes again write contiguous runs).
//
// The user's radix stages (reference: one LDS pass + barrier per stage, one thread per
// output, fft/fft/_ndim_fft_gpu.mojo:359-386) are fused into 2-4 composite passes, e.g.
// 1024 = 2^10 -> 16 * 8 * 8: two LDS exchanges instead of ten.  Work items of a pass are
// flattened over the whole workgroup, so radices that do not divide the thread count
// (31 * 3, 10 * 6 * 8) keep every lane busy.
//
// Strided dimensions (COLS): the tile is TILE adjacent columns, LDS layout [n][column];
// lanes run along the columns, so HBM runs are TILE*8 bytes and LDS accesses are
// contiguous by construction.  The transform is in place -- this replaces the reference's
// transpose kernel + scratch buffer (fft/fft/_ndim_fft_gpu.mojo:210-276, :185).
//
// Twiddles: W_N^n from the plan's fp64-accurate table.  Per-thread twiddles are loop
// invariant over tiles, so a persistent workgroup keeps them in registers (TWMODE 1) or in a
// compact conflict-free LDS table [pass][j][p] (TWMODE 2); TWMODE 0 reads the global table.
// Inverse: conj(F(conj x)) * 1/N with the forward butterflies (bit-identical to conjugated
// twiddles), reference semantics fft/fft/_utils.mojo:101-104, fft/fft/_fft.mojo:292-294.
//
// Real input, N-D plans (the reference computes the whole spectrum in every pass): the LAST pass may transform only the
// columns that are not beyond their mirror image and store every result twice (TileCfg::HERM: contiguous runs of tiles, a
// carried column so that mirrored lines leave whole); the pass in front of it stores only the half it reads (TileCfg::HS),
// or -- three-pass plans -- the first pass does and the middle pass transforms a column prefix (TileParams::col_lim).
// TileCfg::R2C (packed real rows) is the first pass of a half-spectrum forward plan (and a measured tie as the half-store
// first pass of the full-spectrum schedules, kept for the lab build); TileCfg::C2R, its mirror, is the last pass of a
// half-spectrum inverse plan (half_spectrum.cpp).  Selection and policy: mifft_api.cpp, herm_pays().
#pragma once

#include "fft_radix.h"

// cooperative prime pass (bigprime_pass): consecutive output pairs per thread (each input pair is read once per SB outputs)
#ifndef MIFFT_BIGP_SB
#define MIFFT_BIGP_SB 4
#endif

// odd prime radices from this size on use the emit-as-you-go butterfly in LDS-bound passes (pass_compute_scatter): radix 31
// drops from 165 to 145 VGPRs (1023 = 31 * 11 * 3: 0.069 -> 0.055 ms per 128 MB, rows93 real input stops spilling); radices
// 17 / 19 keep all their outputs in registers anyway and measured 0-7 % slower with it (867 = 17 * 17 * 3)
#ifndef MIFFT_EMIT_PRIME_MIN
#define MIFFT_EMIT_PRIME_MIN 23
#endif

namespace mifft {

template <typename T> struct native_vec2;
template <> struct native_vec2<float> { typedef float type __attribute__((ext_vector_type(2))); };
template <> struct native_vec2<double> { typedef double type __attribute__((ext_vector_type(2))); };

// four adjacent reals (DCT tiles): one 16-byte access for float
template <bool NT, typename T>
MIFFT_DEV void gload4(const T* p, T (&v)[4]) {
    typedef T vec4 __attribute__((ext_vector_type(4)));
    vec4 q;
    if constexpr (NT)
        q = __builtin_nontemporal_load((const vec4*)p);
    else
        q = *(const vec4*)p;
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
}
template <bool NT, typename T>
MIFFT_DEV void gstore4(T* p, T a, T b, T c, T d) {
    typedef T vec4 __attribute__((ext_vector_type(4)));
    const vec4 q = {a, b, c, d};
    if constexpr (NT)
        __builtin_nontemporal_store(q, (vec4*)p);
    else
        *(vec4*)p = q;
}

template <bool NT, typename T>
MIFFT_DEV cpx<T> gload(const cpx<T>* p) {
    if constexpr (NT) {
        typename native_vec2<T>::type v = __builtin_nontemporal_load((const typename native_vec2<T>::type*)p);
        return {v.x, v.y};
    } else {
        return *p;
    }
}
template <bool NT, typename T>
MIFFT_DEV T gload_real(const T* p) {
    if constexpr (NT)
        return __builtin_nontemporal_load(p);
    else
        return *p;
}
// two adjacent reals at an address aligned to ONE element (the frames of TileCfg::STFT start at any sample: the hop may be
// odd), as one access that the hardware's unaligned global accesses serve
template <typename T>
MIFFT_DEV cpx<T> gload_pair(const T* p) {
    typedef T vec2u __attribute__((ext_vector_type(2), aligned(sizeof(T))));
    const vec2u v = *(const vec2u*)p;
    return {v.x, v.y};
}
// ... and the store of two adjacent reals at such an address (the rows of a TileCfg::DCT = 4 store)
template <typename T>
MIFFT_DEV void gstore_pair(T* p, T a, T b) {
    typedef T vec2u __attribute__((ext_vector_type(2), aligned(sizeof(T))));
    const vec2u v = {a, b};
    *(vec2u*)p = v;
}
template <bool NT, typename T>
MIFFT_DEV void gstore(cpx<T>* p, cpx<T> v) {
    if constexpr (NT) {
        typename native_vec2<T>::type w = {v.x, v.y};
        __builtin_nontemporal_store(w, (typename native_vec2<T>::type*)p);
    } else {
        *p = v;
    }
}

// one real at an address aligned to one element (the rows of a TileCfg::SPEC store are N + 1 reals wide)
template <bool NT, typename T>
MIFFT_DEV void gstore_real(T* p, T v) {
    if constexpr (NT)
        __builtin_nontemporal_store(v, p);
    else
        *p = v;
}

// the correctly rounded square root (sqrtf / sqrt without a header: this file is also compiled by hipRTC)
MIFFT_DEV float sqrt_t(float v) { return __builtin_sqrtf(v); }
MIFFT_DEV double sqrt_t(double v) { return __builtin_sqrt(v); }

// the full-precision base-2 logarithm (log2f / log2 without a header, as above): the library routine, not v_log_f32 alone
extern "C" __device__ double __ocml_log2_f64(double);
MIFFT_DEV float log2_t(float v) { return __builtin_log2f(v); }
MIFFT_DEV double log2_t(double v) { return __ocml_log2_f64(v); }

template <class A, class B> struct same_t { static constexpr bool value = false; };
template <class A> struct same_t<A, A> { static constexpr bool value = true; };

// The element accesses of a TileCfg::CONV tile, whose rows are stored as ST: T itself -- then these are the plain accesses above,
// instruction for instruction -- or a 16-bit float (_Float16, bf16_t) under T = float.  A load widens exactly; a store rounds
// once, to nearest even (float16: overflow to infinity, subnormals kept; NaN stays NaN).  Pairs are one 4-byte access.
template <typename T, typename ST>
MIFFT_DEV T swiden(ST v) {
    if constexpr (same_t<ST, bf16_t>::value) return (T)(float)v;
    else return (T)v;
}
template <typename ST, typename T>
MIFFT_DEV ST snarrow(T v) {
    if constexpr (same_t<ST, bf16_t>::value) {
        return bf16_t::from_float(v);
    } else {
        if constexpr (same_t<ST, _Float16>::value && !same_t<T, _Float16>::value) {
            // The float the store computed stays a float before it is rounded.  Left to itself the compiler selects
            // v_fma_mixlo_f16 for "postgate * y, then narrow": the exact product rounded ONCE to float16, where the float32
            // kernel followed by a conversion rounds twice -- a different sample about once in 2^13.  An empty statement
            // that only names the register keeps the multiplication and v_cvt_f16_f32 apart (no instruction is emitted).
#if defined(__HIP_DEVICE_COMPILE__)
            asm volatile("" : "+v"(v));
#endif
        }
        return (ST)v;
    }
}
template <typename T, typename ST>
MIFFT_DEV T sload(const ST* p) {
    return swiden<T, ST>(*p);
}
// ... at an address aligned to ONE element, as gload_pair
template <typename T, typename ST>
MIFFT_DEV cpx<T> sload_pair(const ST* p) {
    if constexpr (same_t<ST, T>::value) {
        return gload_pair(p);
    } else {
        static_assert(sizeof(ST) == 2, "16-bit storage");
        typedef unsigned short bits2u __attribute__((ext_vector_type(2), aligned(2)));
        const bits2u v = *(const bits2u*)p;
        const unsigned short lo = v.x, hi = v.y;
        return {swiden<T, ST>(__builtin_bit_cast(ST, lo)), swiden<T, ST>(__builtin_bit_cast(ST, hi))};
    }
}
template <typename ST, typename T>
MIFFT_DEV void sstore(ST* p, T v) {
    *p = snarrow<ST, T>(v);
}
// ... at an address aligned to TWO elements
template <typename ST, typename T>
MIFFT_DEV void sstore_pair(ST* p, T a, T b) {
    if constexpr (same_t<ST, T>::value) {
        gstore<false>((cpx<T>*)p, cpx<T>{a, b});
    } else {
        static_assert(sizeof(ST) == 2, "16-bit storage");
        typedef unsigned short bits2 __attribute__((ext_vector_type(2)));
        const bits2 v = {__builtin_bit_cast(unsigned short, snarrow<ST, T>(a)), __builtin_bit_cast(unsigned short, snarrow<ST, T>(b))};
        *(bits2*)p = v;
    }
}

// one input element of a FOREIGN element type IT (uint8 / int8 / int16 / uint16 / int32 / half / bfloat16, or float under a
// double plan), real or interleaved complex, widened to cpx<T> -- the reference's `x.load(...).cast[out_dtype]()`,
// fft/fft/_fft.mojo:243-257
template <class C>
MIFFT_DEV cpx<typename C::T> load_foreign(const void* in, long long idx) {
    using T = typename C::T;
    using IT = typename C::IT;
    const IT* p = (const IT*)in;
    // through float for bf16_t (its only conversion); exact for every element type narrower than T
    auto widen = [](IT v) -> T {
        if constexpr (same_t<IT, bf16_t>::value) return (T)(float)v;
        else return (T)v;
    };
    if constexpr (C::IN_REAL) {
        return {widen(p[idx]), (T)0};
    } else {
        struct alignas(2 * sizeof(IT)) pair_t { IT re, im; };
        const pair_t v = ((const pair_t*)p)[idx];
        return {widen(v.re), widen(v.im)};
    }
}

struct TileParams {
    const void* in;
    void* out;
    const void* tw;  // cpx<T>[N], conjugated when the plan is an inverse plan
    long long n_tiles;
    long long n_rows;           // ROWS
    long long inner;            // COLS
    long long tiles_per_outer;  // COLS
    int inverse;
    double scale;  // 1/N for inverse
    // TSTORE configurations (first pass of the four-step): two-level table of W_M^m, M = N * inner,
    // W_M^m = tlo[m mod 1024] * thi[m div 1024]
    const void* tlo;
    const void* thi;
    const void* tcol;  // [TILE][N]: W_M^(c * k1), the twiddle of column c0 + c relative to column c0
    // walk the tiles from the last to the first.  An in-place pass that follows a pass over the same tensor then
    // starts with the lines written LAST, i.e. the ones most likely to be still in the 256-MiB Infinity Cache (LRU:
    // walking forward again would evict exactly the lines it is about to need).
    int reverse;
    // FS1 configurations: `inner` is the LOAD row stride N2 * fs_inner; rows are stored at stride fs_inner
    long long fs_inner;
    long long fs_n2;
    // HERM configurations (last pass of a REAL-input N-D plan, in place): herm_d0 x herm_d1 x herm_d2 are the trailing
    // dimensions, i.e. the column space (leading ones 1 when absent).  One of them is the HALF AXIS (size herm_dj, stride
    // herm_js columns): the pass transforms the columns whose index along it is at most herm_dj / 2 and owns those below the
    // middle.  The column space is herm_rows rows of herm_L = herm_dj * herm_js columns; the first herm_H = (herm_dj / 2 + 1)
    // * herm_js columns of every row are covered by herm_tpr tiles, tiles_per_outer = rows * herm_tpr.
    union { int herm_d0; int conv_Q; };      // PART: taps per partition
    union { int herm_d1; int conv_parts; };  // PART: partitions of the filter
    int herm_d2;
    int herm_dj, herm_js, herm_L, herm_H, herm_tpr;
    // HS configurations (the pass BEFORE a HERM last pass; a plane: its column side): results with an output index above
    // store_lim are not stored -- the last pass reads only the half of that dimension up to its middle and writes the rest
    int store_lim;
    // R2C / C2R configurations: W_(2N)^k, k = 0 .. N (forward, whatever the plan's direction), and the row pitch (complex
    // elements) of the half-spectrum side: `out` of R2C (2 N in a full-spectrum plan, N + 1 in a half-spectrum one), `in` of C2R
    const void* r2c_tw;
    long long half_pitch;
    // column tiles of a pass that transforms only a PREFIX of its column space (the middle pass of a half-spectrum schedule):
    // columns from col_lim on are neither loaded nor stored (0 = all `inner` columns)
    long long col_lim;
    // DCT configurations: W_(4n)^k = e^(-2 pi i k / 4n), k = 0 .. N (n = 2 N real points per row), and the scales of bin 0 and
    // of the other bins (the norm, the factor 2 of the forward, the 1 / 2n and the halves of the inverse): applied as the
    // bins are stored (DCT = 2) or loaded (DCT = 3).  DCT = 4: dct_tw holds p_m = e^(-i pi (8m+1) / 8n), m = 0 .. N - 1, the
    // pre- and the post-twiddle alike, and dct_s1 the one scale of the store (dct_s0 is unused).  MDCT configurations reuse the
    // STFT fields below: frames of 4 N samples every stft_hop = 2 N, stft_win their 4 N window values, stft_center = 2.
    const void* dct_tw;
    double dct_s0, dct_s1;
    // STFT configurations: logical row r of the launch is frame r % stft_frames of batch entry r / stft_frames, entries of
    // stft_len reals; the frame starts at sample frame * stft_hop - (stft_center ? N : 0) of its entry (N = half the frame
    // length) and is multiplied by stft_win, 2 N values of type T.  stft_center: 0 no frame leaves its entry, 1 the signal is
    // reflected at both ends (N <= stft_len - 1: one reflection), 2 zeros beyond both ends.
    const void* stft_win;
    union { int stft_frames; int conv_Lo; };  // CONV: output samples per (signal) row, the pitch of `out` and gate_out
    union { int stft_hop; int conv_o; };      // CONV: the first stored sample of every (block's) circular result, o / c
    union { int stft_len; int conv_len; };    // CONV: samples per input row, L / T, the pitch of `in` and gate_in
    union { int stft_center; int conv_D; };   // CONV: filter rows; row r takes filter row r % D
    // ISTFT configurations reuse the four integers (frames per entry F, hop, output samples per entry T, centred or not) and
    // stft_win (the synthesis table, below); tiles_per_outer is the tiles of ONE entry, ceil(F / TILE), and istft_env the
    // reciprocal envelope 1 / sum w^2 at every padded sample 0 .. 2 N + hop (F - 1) - 1, type T.  STFT tiles with IADJ (the
    // adjoint of the inverse STFT) read the same table in their load.
    const void* istft_env;
    // SPEC configurations with a filterbank (TileCfg::FB): band m < spec_bands is sum_j spec_wt[spec_off[m] + j] *
    // P[spec_lo[m] + j], j < spec_len[m] (spec_lo[m] + spec_len[m] <= N + 1; weights of type T).  Without one the four
    // pointers are null and spec_bands is 0.
    // CONV: the filter spectra, (D[, parts], N + 1) complex values of type T; WGRAD (which has no filter): the pregate
    // ISTFT tiles with ADJ >= 2 (the adjoint of a spectrogram): adj_mult, the real per-bin factor, rows of N + 1 values of type T
    // beside the rows of `in`
    union { const void* spec_wt; const void* conv_h; const void* wgrad_pregate; const void* adj_mult; };
    const int* spec_lo;
    const int* spec_len;
    const int* spec_off;
    // CONV: the first (signal) row of the launch modulo D; WGRAD: the partial sums per channel, P
    union { int spec_bands; int conv_row0; int wgrad_partials; };
    // LOG configurations: y = fma(spec_a, log2(max(v + spec_add, spec_amin)), spec_c) on every value the SPEC / FB store
    // would have written; the four are exact values of type T (spec_amin a normal one, so the logarithm sees no denormal).
    // POST configurations (with FB): spec_post is a dense, row-major (spec_bands, spec_q) matrix of type T applied to the
    // bands of every frame, spec_bands <= N - 1; the store writes spec_q reals per frame.
    double spec_add, spec_amin, spec_a, spec_c;
    // ISTFT tiles with ADJ (the adjoint of the STFT; stft_center 1 = reflect, 2 = zeros): adj_edge, (entries, 2, N) values of
    // type T, the padded samples before (side 0) and behind (side 1) the entry's stft_len stored ones, written when
    // stft_center is 1; null otherwise.  An exec's argument, as `out` is.
    union { const void* spec_post; void* adj_edge; };
    union { int spec_q; int conv_mode; };  // CONV: bit 0 = correlate (multiply by the conjugate)
    // CONV configurations (an R2C tile that is neither STFT nor SPEC) read the conv_* names declared above on the bytes of
    // fields no such tile uses otherwise, so that the layout of the kernel argument stays what every other kernel was built
    // for.  Every form sets conv_len, conv_o, conv_Lo, conv_D, conv_h, conv_mode and conv_row0: the samples o .. o + Lo - 1
    // of every result are stored, row r of the launch against filter row (conv_row0 + r) % D.  scale is 1 / 2N; inverse is 0.
    // OLS configurations add the three fields below: launch row r is block r % ols_blocks of signal r / ols_blocks; block f
    // loads the 2N samples from ols_start + f * ols_step on (zeros outside [0, conv_len)) and stores the samples
    // conv_o .. conv_o + ols_step - 1 of its result to out[f * ols_step ..] of its signal's row, up to conv_Lo.  conv_row0
    // counts signals, not launch rows.
    // PAIR configurations (two signals: TileCfg::PAIR) read three other names on the same bytes: pair_K the samples per row of
    // v, pair_ea / pair_eb the index at which a row of x / of v starts inside its 2N zero-extended samples.  v itself is
    // gate_in (rows of pair_K reals, at the exec's first row as `in` is); conv_h, conv_D and conv_row0 are unused.
    union { int ols_step; int pair_K; };
    union { int ols_blocks; int pair_ea; };
    union { int ols_start; int pair_eb; };
    // WGRAD configurations (the filter gradient of CONV / OLS) always carry the three ols_* fields (a single block:
    // ols_blocks = 1, ols_start = 0, ols_step = Lo) and wgrad_partials = P in the place of conv_row0; there is no filter.  `in`
    // is x, gate_in is gy (rows of conv_Lo reals), n_rows the pairs of ONE channel, B F: workgroup w is slice w % P of channel
    // w / P and stores row (w % P) D + w / P of `out`, (P D) rows of N + 1 complex values.  With GATE the gates of the forward
    // plan multiply the two inputs as they are loaded: wgrad_pregate (in the place of conv_h; x's shape) every sample of x,
    // gate_out (gy's shape: the forward's `out`) every sample of gy; null where there is no such gate.
    // WSPEC configurations (WGRAD's store variant) read the same fields; `out` is (rows, ols_blocks, N + 1) complex values
    // and wgrad_partials only slices the walk.  WSPEC = 1 never reads gate_in / gate_out, WSPEC = 2 never `in` / wgrad_pregate.
    // PART configurations (partitioned overlap-save) are OLS's with conv_Q and conv_parts set.
    // GATE configurations (CONV / OLS / PART with elementwise gates; the arguments of one exec, not plan state): gate_in has
    // the shape of `in` and multiplies every sample as it is loaded, gate_out the shape of `out` and multiplies every sample as
    // it is stored.  Both point, as `in` and `out` do, at the exec's first signal row; null where there is no such gate.
    const void* gate_in;
    const void* gate_out;
};
// (the conv_* names are other names of the same bytes: nothing moves)
static_assert(sizeof(TileParams) == 352 && __builtin_offsetof(TileParams, conv_Q) == __builtin_offsetof(TileParams, herm_d0) &&
                  __builtin_offsetof(TileParams, conv_o) == __builtin_offsetof(TileParams, stft_hop) &&
                  __builtin_offsetof(TileParams, conv_h) == __builtin_offsetof(TileParams, spec_wt) &&
                  __builtin_offsetof(TileParams, wgrad_pregate) == __builtin_offsetof(TileParams, conv_h) &&
                  __builtin_offsetof(TileParams, adj_mult) == __builtin_offsetof(TileParams, spec_wt) &&
                  __builtin_offsetof(TileParams, adj_edge) == __builtin_offsetof(TileParams, spec_post) &&
                  __builtin_offsetof(TileParams, wgrad_partials) == __builtin_offsetof(TileParams, spec_bands) &&
                  __builtin_offsetof(TileParams, conv_mode) == __builtin_offsetof(TileParams, spec_q) &&
                  __builtin_offsetof(TileParams, pair_K) == __builtin_offsetof(TileParams, ols_step) &&
                  __builtin_offsetof(TileParams, pair_ea) == __builtin_offsetof(TileParams, ols_blocks) &&
                  __builtin_offsetof(TileParams, pair_eb) == __builtin_offsetof(TileParams, ols_start),
              "TileParams: a CONV name left the field it shares");

// the log stage of a TileCfg::LOG store: fma(a, log2(max(v + add, amin)), c)
template <typename T>
MIFFT_DEV T spec_log(const TileParams& p, T v) {
    const T s = v + (T)p.spec_add, lim = (T)p.spec_amin;
    return fma_t((T)p.spec_a, log2_t(s < lim ? lim : s), (T)p.spec_c);  // (a NaN stays one, as through torch.clamp)
}

MIFFT_DEV long long tile_id(const TileParams& p, long long t) { return p.reverse ? p.n_tiles - 1 - t : t; }

constexpr int ilog2_ce(int v) {
    int l = 0;
    while ((1 << (l + 1)) <= v) ++l;
    return l;
}
constexpr bool is_pow2_ce(int v) { return v > 0 && (v & (v - 1)) == 0; }

enum { TW_GLOBAL = 0, TW_REG = 1, TW_LDS = 2 };

// ---- Rader: a prime radix R too large for a register butterfly (R > 32) as a cyclic convolution of length M = R - 1 ----
// x[g^q] (*) W_R^(g^-q), computed with an M-point FFT, a pointwise product with the precomputed spectrum of the kernel and
// an inverse M-point FFT, all inside the LDS tile (rader_pass).  2 * 5 M log2 M flops per R-point DFT instead of the 4 (R/2)^2
// FMAs of the cooperative conjugate-pair pass (bigprime_pass): 3x fewer at R = 97, 20x at R = 1009.  Applicable when
// M = R - 1 splits into at most four register butterflies (factors <= 16, or one prime <= 31 each): rader_ok, evaluated by
// the host, which selects the pass per configuration (TileCfg::RADERM) and uploads its tables.
struct RaderSplitT {
    int np;
    int r[4];
    bool ok;
};
constexpr RaderSplitT rader_split(int M) {
    RaderSplitT s{0, {1, 1, 1, 1}, false};
    int pf[32] = {};
    int npf = 0, m = M;
    for (int d = 2; d <= m; ++d)
        while (m % d == 0) {
            if (npf >= 32) return s;
            pf[npf++] = d;
            m /= d;
        }
    bool used[32] = {};
    int left = npf;
    while (left > 0) {
        if (s.np >= 4) return s;
        int r = 1;
        for (int i = npf - 1; i >= 0; --i) {
            if (used[i]) continue;
            if (r == 1) {
                if (pf[i] > 31) return s;
                r = pf[i];
            } else if (r * pf[i] <= 16) {
                r *= pf[i];
            } else {
                continue;
            }
            used[i] = true;
            --left;
        }
        s.r[s.np++] = r;
    }
    s.ok = s.np >= 1;
    return s;
}
constexpr bool rader_ok(int R) { return R > 32 && rader_split(R - 1).ok; }
// R - 1 with a prime factor above 31 (83, 509, 2039 ...): the cyclic convolution of length M = R - 1 is embedded in one of
// length L >= 2 M - 1 (zero-padded sequence, wrapped kernel) with L a product of factors <= 16; it runs in a scratch block
// of L elements per DFT beside the data tile.  0 = none below 8192.
constexpr bool rader_small_radices(int L) {
    const RaderSplitT s = rader_split(L);
    if (!s.ok) return false;
    for (int i = 0; i < s.np; ++i)
        if (s.r[i] > 16) return false;
    return true;
}
constexpr int rader_pad_len(int R) {
    for (int L = 2 * (R - 1) - 1; L <= 8192; ++L)
        if (rader_small_radices(L)) return L;
    return 0;
}
// convolution length of a Rader pass: M in place, or the padded L
constexpr int rader_len(int R) { return rader_ok(R) ? R - 1 : rader_pad_len(R); }
// LDS of one Rader pass in units of one complex element of `esz` bytes: spectrum of the kernel [M], W_M [M], the two
// permutations (2 M uint16) and x_0 of every R-point DFT of the tile [inst]
// (+ the scratch blocks of a padded pass: inst * L)
constexpr int rader_lds_elems(int R, int inst, int esz) {
    const int L = rader_len(R);
    return 2 * L + (4 * (R - 1) + esz - 1) / esz + inst + (rader_ok(R) ? 0 : inst * L);
}

template <typename T_, int N_, int NP_, int R0_, int R1_, int R2_, int R3_, int TILE_, int THREADS_, bool COLS_,
          bool FIRST_DIRECT_, bool LAST_DIRECT_, int TWMODE_, int MINW_ = 1, bool PREFETCH_ = false, int ROWPAD_ = 0,
          bool IN_REAL_ = false, bool DMA_ = false, int NT_ = 0, bool TSTORE_ = false, typename IT_ = T_, bool WSUB_ = false,
          bool FS1_ = false, int RADERM_ = 0, bool HERM_ = false, bool HS_ = false, bool R2C_ = false, bool C2R_ = false,
          int ILV_ = 0, int DCT_ = 0, bool STFT_ = false, bool ISTFT_ = false, int SPEC_ = 0, bool FB_ = false,
          bool LOG_ = false, bool POST_ = false, bool MDCT_ = false, bool IMDCT_ = false, bool DST_ = false,
          bool CONV_ = false, bool OLS_ = false, int GATE_ = 0, bool WGRAD_ = false, bool PART_ = false,
          int ADJ_ = 0, bool IADJ_ = false, int WSPEC_ = 0, bool PAIR_ = false>
struct TileCfg {
    using T = T_;
    static constexpr int N = N_, NP = NP_, TILE = TILE_, THREADS = THREADS_, TWMODE = TWMODE_, MINW = MINW_;
    static constexpr bool COLS = COLS_, FIRST_DIRECT = FIRST_DIRECT_, LAST_DIRECT = LAST_DIRECT_;
    static constexpr bool PREFETCH = PREFETCH_ && FIRST_DIRECT_;
    // pass 0 reads a REAL tensor (C_in = 1) and promotes it (fft/fft/_fft.mojo:254-255).  Compile-time:
    // a runtime switch inside the prefetching load loop cost 0.30 -> 0.49 ms at 100k x 1024.
    static constexpr bool IN_REAL = IN_REAL_;
    // element type of the tensor pass 0 reads (the plan's in_dtype): T itself, or uint8 / int32 / float widened to T
    // in the load (the reference's `x.load(...).cast[out_dtype]`, fft/fft/_fft.mojo:243-251).  Only the
    // runtime-specialised kernels (kernels_jit.cpp) instantiate foreign input types.
    using IT = IT_;
    // non-temporal HBM accesses (bit 0: loads, bit 1: stores).  A tile is read once and written once; the
    // streaming hint lifts a row-shaped copy from ~5.85 to ~6.4 TB/s on MI355X (tools/micro/copy_nt.hip) when
    // the tensors dwarf the 256-MB Infinity Cache, and HURTS cache-resident or in-place passes (measured:
    // N = 93 flat copy 0.173 -> 0.247 ms, 640-point column tiles 0.114 -> 0.139 ms), so it is a twin
    // configuration chosen at plan time by tensor size.
    static constexpr int NT = NT_;
    static constexpr int LD = N_ + ROWPAD_;  // ROWS: LDS pitch of one transform
    static constexpr int R(int i) { return i == 0 ? R0_ : i == 1 ? R1_ : i == 2 ? R2_ : R3_; }
    static constexpr int P(int i) {
        int p = 1;
        for (int k = 0; k < i; ++k) p *= R(k);
        return p;
    }
    static constexpr int NB(int i) { return N / R(i); }
    static constexpr int ITEMS(int i) { return NB(i) * TILE; }
    // WSUB (column tiles): after pass 0 (radix R0) the transform falls apart into R0 independent sub-problems -- the
    // elements at positions = p (mod R0) -- and every later pass works inside them.  With WSUB a wave OWNS SPW of these
    // sub-problems (all TILE columns) for the passes 1..NP-1, so the exchanges between those passes touch only LDS
    // positions of its own sub-problems: one wave's LDS instructions execute in order and no workgroup barrier is
    // needed.  Two workgroup barriers per tile remain (after the pass-0 scatter, after the last gather) instead of
    // 2 (NP - 1); the waves drift apart and overlap each other's butterflies, LDS traffic and HBM stores.
    static constexpr bool WSUB = WSUB_;
    static constexpr int WAVES = THREADS_ / 64;
    static constexpr int SPW = WSUB_ ? R0_ / (WAVES > 0 ? WAVES : 1) : 1;  // sub-problems per wave
    static constexpr int WSLOTS = 64 / (TILE_ <= 64 ? TILE_ : 64);        // (sub-problem, butterfly) pairs per wave instruction
    static constexpr int WPER(int i) { return SPW * (NB(i) / R0_); }      // ... per wave and pass
    static_assert(!WSUB_ || (COLS_ && THREADS_ % 64 == 0 && 64 % TILE_ == 0 && R0_ % (THREADS_ / 64) == 0 && !TSTORE_ &&
                             TWMODE_ != TW_REG && NP_ >= 2 && FIRST_DIRECT_ && LAST_DIRECT_ && R0_ <= 32),
                  "WSUB: column tile, TILE divides a wave, R0 a multiple of the wave count");
    static constexpr int IPT(int i) {
        return (WSUB_ && i >= 1) ? (WPER(i) + WSLOTS - 1) / WSLOTS : (ITEMS(i) + THREADS - 1) / THREADS;
    }
    static constexpr int TW_OFF(int i) {  // register twiddles of passes 1..i-1 precede pass i
        int o = 0;
        for (int k = 1; k < i; ++k) o += IPT(k) * (R(k) - 1);
        return o;
    }
    static constexpr int TW_TOTAL = TW_OFF(NP_);
    static constexpr int TWL_OFF(int i) {  // compact LDS table [pass][j-1][p]
        int o = 0;
        for (int k = 1; k < i; ++k) o += P(k) * (R(k) - 1);
        return o;
    }
    static constexpr int TWL_TOTAL = TWMODE_ == TW_LDS ? TWL_OFF(NP_) : 0;
    // TSTORE (column tiles only): the finished tile is stored TRANSPOSED and multiplied by the four-step twiddle
    // W^{k1*n2}: columns c0..c0+TILE-1 of the [N][inner] matrix become TILE contiguous rows of the [inner][N]
    // matrix, so the store is one flat coalesced run.  The LDS column pitch is TILE + 1 so that the transposed
    // read (lanes along n) is conflict-free.
    // Re-derive every thread-index-dependent offset inside each tile iteration instead of letting the compiler
    // hoist them out of the persistent loop (see tile_kernel).  Column tiles and very long rows carry dozens of
    // such offsets and spill or lose occupancy when they stay live; the short-row kernels run at copy speed with
    // them hoisted and lose 3-8 % to the recomputation (A/B on MI355X, gpurun_out/ab_opaque.log).
#ifdef MIFFT_OPAQUE_ROWS
    static constexpr bool OPAQUE_TID = true;
#else
    static constexpr bool OPAQUE_TID = COLS_ || N_ >= 8192;
#endif
    // Tile -> workgroup mapping.  Workgroups are dealt round-robin to the 8 XCDs (workgroup id mod 8), each with its
    // own L2.  Column tiles whose runs are NARROWER than a 128-B line (long strided dimensions: 8 / 4 columns) give
    // every XCD one CONTIGUOUS eighth of the tiles, so that the two / four tiles sharing a line meet in one L2 instead
    // of each XCD fetching and writing the line partially: 8-column tiles gain 10 %, 4-column tiles 24-36 % (4K frame
    // 0.104 -> 0.078 ms).  Full-line tiles (16 columns) are mixed under the same mapping -- 640 / 128 / 256-point tiles
    // gain 3-7 %, the 2^20 four-step and 64^3 lose 6 % (same-box A/B) -- and row tiles are neutral, so
    // both keep the plain round-robin order.
#ifdef MIFFT_NO_XCD_CHUNK
    static constexpr bool XCD_CHUNK = false;
#else
    static constexpr bool XCD_CHUNK = COLS_ && TILE_ * 2 * (int)sizeof(T_) < 128;
#endif
    static constexpr bool TSTORE = TSTORE_;
    // FS1 (column tiles): first pass of the four-step of a STRIDED dimension of N = N1 * N2 points (N1 = this
    // configuration's N).  The dimension is viewed as [N1][N2] rows of `fs_inner` contiguous elements; the tile of
    // (n2, 16 columns) is transformed over n1 (row stride N2 * fs_inner) and its row k1 is stored, multiplied by
    // W_N^(k1 * n2), as row n2 * N1 + k1 of the OTHER buffer -- a row-granular transposition, so the stores keep their
    // TILE-element runs and need no LDS round trip.  The second pass (an ordinary column tile of N2 points at row
    // stride N1 * fs_inner) then leaves the spectrum in natural order.
    static constexpr bool FS1 = FS1_;
    // HERM (column tiles, in place): the LAST pass of a real-input N-D transform.  The spectrum of a real tensor is
    // Hermitian, Y[-k, -c] = conj(Y[k, c]) over the transformed dimensions, and so is every intermediate over the dimensions
    // already transformed: column -c of this pass holds the conjugate of column c.  Only the columns c <= -c (a flat prefix
    // of the column space) are read and transformed; every result is stored twice, at (k, c) and conjugated at (-k, -c).
    // Half the reads and butterflies of the pass; the reference computes (and this library's other kernels compute) all of it.
    static constexpr bool HERM = HERM_;
    static_assert(!HERM_ || (COLS_ && LAST_DIRECT_ && !TSTORE_ && !FS1_), "HERM: a direct in-place column tile");
    // HS ("half store"): the pass that transforms the dimension a following HERM pass halves -- the one before the last of a
    // real-input N-D plan -- stores only the results 0 .. store_lim (= N / 2) of every transform: the HERM pass reads nothing
    // else and writes every other point itself.  Half the writes of that pass.
    static constexpr bool HS = HS_;
    static_assert(!HS_ || (!TSTORE_ && !FS1_ && !HERM_), "HS: a plain row / column tile or the column side of a plane");
    // R2C: a row tile over a REAL tensor whose rows of 2 N points are read as N packed complex points z_n = x_2n + i x_2n+1
    // (the row as it lies in memory), transformed by the ordinary passes, and unpacked into X[0 .. N] of the 2 N-point real
    // transform by the store loop (the classic real-FFT split): half the butterflies and LDS traffic of a promoted (x, 0)
    // row.  Only the half spectrum is produced, so it serves where a Hermitian last pass follows (it is a half-store kernel).
    static constexpr bool R2C = R2C_;
    static_assert(!R2C_ || (!COLS_ && !LAST_DIRECT_ && !IN_REAL_ && !TSTORE_ && !FS1_ && !HERM_ && !HS_ && !DMA_),
                  "R2C: a row tile that leaves its last pass in LDS");
    // C2R: the mirror of R2C, the last pass of a half-spectrum inverse.  A row of N + 1 bins X[0 .. N] of a 2 N-point REAL
    // signal is folded into the N-point spectrum Z[k] = E[k] + i O[k] of the packed row z_n = x_2n + i x_2n+1 as it is loaded
    // (E[k] = X[k] + conj X[N-k], O[k] = (X[k] - conj X[N-k]) W^-k, W = e^(-2 pi i / 2N); the imaginary parts of X[0] and X[N]
    // are ignored, as numpy's irfft does), transformed back by the ordinary passes and stored as a plain row of N complex =
    // 2 N reals with the scale 1 / 2N of the plan's pass.  Half the butterflies of a complex row.
    static constexpr bool C2R = C2R_;
    static_assert(!C2R_ || (!COLS_ && !FIRST_DIRECT_ && !IN_REAL_ && !TSTORE_ && !FS1_ && !HERM_ && !HS_ && !DMA_ && !R2C_ &&
                            same_t<IT_, T_>::value && R0_ <= 32),
                  "C2R: a row tile whose pass 0 reads the folded row from LDS");
    // inverse plans run conj(F(conj x)): complex input is conjugated as it is loaded (a real input is its own conjugate; the
    // packed rows of R2C are unpacked first and conjugated as they are stored; C2R conjugates the folded row it writes)
    static constexpr bool CONJ_IN = !IN_REAL_ && !R2C_ && !C2R_;
    static_assert(!FS1_ || (COLS_ && FIRST_DIRECT_ && LAST_DIRECT_ && !TSTORE_ && !WSUB_), "FS1: a direct column tile");
    // ILV (interleaved blocks, I = ILV_ > 0): a row-shaped tile over TILE / I consecutive blocks of an (outer, N, I) tensor
    // -- the pass over a dimension whose kept trailing dimensions hold I < 128 B of elements.  Transform t = g * I + c of the
    // tile takes element n from flat index g * N * I + n * I + c of its block run: the tile's footprint is ONE flat run of
    // TILE * N elements, copied HBM <-> LDS by the flat loops (every wave access contiguous), and the stride-I gather into
    // the per-transform rows of LDS happens on the LDS side.  ROWPAD_ spreads the I transforms a 16-lane group of the copy
    // touches over the banks (kernels_jit.cpp, ilv_rowpad).  The passes are the row tile's.
    static constexpr int ILV = ILV_;
    static_assert(!ILV_ || (!COLS_ && !FIRST_DIRECT_ && !LAST_DIRECT_ && TILE_ % ILV_ == 0 && !TSTORE_ && !FS1_ && !HERM_ &&
                            !HS_ && !R2C_ && !C2R_ && !DMA_ && R0_ <= 32),
                  "ILV: a row tile of whole blocks staged by the flat copies");
    // DCT (2 / 3; 0 = none): DCT-II of real rows of n = 2 N points on the packed-row kernels, by Makhoul's route.  The row
    // v[j] = x[2j], v[n-1-j] = x[2j+1] is a real sequence whose transform V gives X[k] = 2 Re(W_4n^k V[k]) and
    // X[n-k] = -2 Im(W_4n^k V[k]).  2: an R2C tile whose load scatters x into the real slots of v (slot q is component
    // q & 1 of complex element q >> 1: the packed row of v lies in LDS with no staging) and whose unpacking loop, holding
    // V[k] and V[N-k], multiplies by the quarter-sample twiddle and stores four runs of reals.  3, the inverse: a C2R
    // tile whose load forms V[k] = conj(W_4n^k) (X[k] - i X[n-k]) / 2 from four runs of reals before the fold, and whose
    // store reads x back from the slots of v.  n reals read once, n reals written once.
    static constexpr int DCT = DCT_;
    static_assert(DCT_ == 0 || DCT_ == 2 || DCT_ == 3 || DCT_ == 4, "DCT: 0, 2 (DCT-II), 3 (its inverse) or 4 (DCT-IV)");
    // DCT = 4: DCT-IV of real rows of n = 2 N points, X[k] = s / 2 * 2 sum_j x[j] cos(pi (2j+1)(2k+1) / 4n), as ONE N-point
    // complex transform between two twiddles.  z_m = x[2m] + i x[n-1-2m], S = p . F(p . z) with p_m = e^(-i pi (8m+1) / 8n)
    // (TileParams::dct_tw), X[2k] = s Re S_k and X[n-1-2k] = -s Im S_k.  A row tile that is neither R2C nor C2R: the load
    // stages p . z in LDS, the passes are the forward complex row's and leave Z in LDS, the store multiplies by p again.
    // Work item m < ceil(N / 2) of the load takes the adjacent pairs (x[2m], x[2m+1]) and (x[n-2-2m], x[n-1-2m]) -- one wave
    // access ascending, one descending, both contiguous -- which are z_m = (x[2m], x[n-1-2m]) and z_(N-1-m) =
    // (x[n-2-2m], x[2m+1]), and writes two whole LDS elements; the store is the mirror: from c_k = p_k Z_k and c_(N-1-k)
    // the pairs (X[2k], X[2k+1]) = (s Re c_k, -s Im c_(N-1-k)) and (X[n-2-2k], X[n-1-2k]) = (s Re c_(N-1-k), -s Im c_k).
    // The middle item of an odd N is its own partner.  The transform is its own inverse up to the scale s, so the plan's
    // direction conjugates nothing (the host passes inverse = 0 and the forward tables).  n reals read once, n written once;
    // the accesses are aligned to one element at least, as the DCT-II rows'.
    static_assert(DCT_ != 4 || (!COLS_ && !R2C_ && !C2R_ && !FIRST_DIRECT_ && !LAST_DIRECT_ && !IN_REAL_ && !TSTORE_ && !FS1_ &&
                                !HERM_ && !HS_ && !DMA_ && !ILV_ && same_t<IT_, T_>::value && R0_ <= 32 && ROWPAD_ >= 0),
                  "DCT-IV: a complex row tile of the plan's own float type, staged in LDS by the twiddling load");
    // MDCT (with DCT = 4): the rows are the lapped FRAMES of a signal.  Frame f of an entry of stft_len samples covers the
    // samples [(f - 1) M, (f + 1) M), M = 2 N coefficients per frame, zeros outside [0, T) without a load; its 2 M windowed
    // samples y are folded to u[i] = -y[3h-1-i] - y[3h+i], u[h+i] = y[i] - y[M-1-i] (i < h = M / 2) as they are loaded, and
    // u takes the place of the DCT-IV row x.  The split of the tile's first row into (entry, frame) and the wrap into the
    // following entries are the STFT load's.  A frame inside its entry forms its four values of u from four pair loads of
    // the signal and of the window, two ascending and two descending; a frame that reaches beyond either end -- and the
    // middle item of an odd h, whose pairs straddle a quarter boundary -- goes real by real with bounds tests.  The choice
    // is per row, so a frame's result does not depend on batch, slab or grid.  The store is the DCT-IV store, rows of M reals.
    static constexpr bool MDCT = MDCT_;
    static_assert(!MDCT_ || DCT_ == 4, "MDCT: the framing, folding load of a DCT-IV tile");
    // IMDCT (with DCT = 4): the inverse.  The rows are TILE consecutive frames of M = 2 N coefficients of ONE batch entry (the
    // tiles, the ascending runs and the ragged last tile of an entry are the ISTFT's); load and passes are the DCT-IV's.  The
    // store first finishes the DCT-IV in place -- one sweep replaces Z_k by c_k = p_k Z_k, so that v[2k] = Re c_k and
    // v[M-1-2k] = -Im c_k are the plain cosine sums of the frame -- and then has one work item per PAIR of output samples of
    // the tile's blocks.  Block q of an entry is out[q M + i], i < M: acc = ws[M+i] y_q[M+i], out = fma(ws[i], y_(q+1)[i], acc),
    // the term of the earlier frame first, with the unfold y[i] = v[h+i], y[M-1-i] = -v[h+i], y[3h-1-i] = -v[i],
    // y[3h+i] = -v[i] (i < h = N) read straight from the slots of v: no frame of 2 M samples exists anywhere.  ws (stft_win,
    // 2 M values) is gain * w; dct_s1 is not applied.  The second half of frame q is a function of v_q[0 .. h) alone: the last
    // frame of a tile leaves those h reals in `carry` (behind the tables) AFTER every read of the previous carry, a barrier
    // between them; the first tile of an entry reads none (frame 0 gives only its second half, to block 0) and the last one
    // writes none.  A run that starts inside an entry at tile g first transforms ONE frame, g TILE - 1, with the stores
    // suppressed, and takes its carry from it.  Every sample of [0, T) is written exactly once with a plain store (pairs; a
    // tail of one real), from the same two products whatever the batch, slab, grid and run layout.
    static constexpr bool IMDCT = IMDCT_;
    static_assert(!IMDCT_ || (DCT_ == 4 && !MDCT_), "IMDCT: the unfolding, overlap-adding store of a DCT-IV tile");
    //
    // DCT on a COLUMN tile (N-D DCT plans, dctn.cpp): the dimension is n = N points at a stride of S reals, S even, and the
    // tile's complex element at stride S / 2 is a PAIR of adjacent real columns, u = x_a + i x_b.  2: the rows of the tile are
    // permuted as they are loaded (v[j] = u[2j], v[N-1-j] = u[2j+1]: in the direct pass-0 load, or by the staging copy when
    // !FIRST_DIRECT), Z = F(v) stays in LDS, and the store loop -- one thread per pair of rows (k, N - k) and column --
    // separates V_a = (Z[k] + conj Z[N-k]) / 2 and V_b = (Z[k] - conj Z[N-k]) / 2i, multiplies both by W_4n^k and stores
    // row k as (s Re t_a, s Re t_b) and row N - k as (-s Im t_a, -s Im t_b).  3: the load combines rows k and N - k into
    // Z[k] = conj(W_4n^k) (s_k U[k] - i s U[N-k]) and Z[N-k] in LDS (U[N] := 0), the passes run the inverse transform and
    // the last pass stores element j straight to row 2j or 2 (N-1-j) + 1.  Every length N >= 2, odd ones included; every
    // HBM access is a run of TILE adjacent elements.
    static_assert(DCT_ != 2 || (COLS_ ? !LAST_DIRECT_ : (R2C_ && !FIRST_DIRECT_)),
                  "DCT-II: packed real rows staged in LDS by the permuting load, or a paired-column tile whose last pass stays in LDS");
    static_assert(DCT_ != 3 || (COLS_ ? (!FIRST_DIRECT_ && LAST_DIRECT_) : (C2R_ && !LAST_DIRECT_)),
                  "inverse DCT-II: folded rows whose last pass stays in LDS, or a paired-column tile combined in LDS");
    static_assert(!(DCT_ != 0 && COLS_) || (!R2C_ && !C2R_ && !IN_REAL_ && !TSTORE_ && !FS1_ && !HERM_ && !HS_ && !DMA_ && !WSUB_ &&
                                            !ILV_ && same_t<IT_, T_>::value && R0_ <= 32 && R1_ <= 32),
                  "DCT on a column tile: a plain in-place tile of register butterflies over pairs of real columns");
    // DST (with DCT = 2 / 3 / 4): the sine transform of the same type on the same tile.  With xs[j] = (-1)^j x[j], the DST-II is
    // Y[k] = 2 sum_j x[j] sin(pi (k+1)(2j+1) / 2n) = DCT-II(xs)[n-1-k] and the DST-IV Y[k] = DCT-IV(xs)[n-1-k]: a sign where
    // the samples are loaded (forward) or stored (inverse) and the index reversal where the bins are stored (forward) or
    // loaded (inverse).  Passes, tables and scales are the DCT's; dct_s0 lands on the LAST bin.
    //   rows, DCT = 2: the permuting load negates the odd samples (the quad's whole element z_(N-1-e)); the unpacking store
    //     writes X[k] to n-1-k (descending), X[n-k] to k-1 (ascending), X[N-k] to N-1+k and X[N+k] to N-1-k: four runs still.
    //   rows, DCT = 3: the four-run load reads X[j] from n-1-j; the store negates the odd samples as it reads the slots of v.
    //   rows, DCT = 4: n is even, so x[n-1-2m] is an odd sample: z_m = x[2m] - i x[n-1-2m], and the store writes
    //     out[2k] = -s Im c_k and out[n-1-2k] = s Re c_k.  No address changes.
    //   columns, DCT = 2: row j of the pair takes (-1)^j as it is loaded, bin k is stored to row N-1-k.
    //   columns, DCT = 3: bins k and N-k are read from rows N-1-k and k-1; the last pass negates what it stores to an odd row.
    static constexpr bool DST = DST_;
    static_assert(!DST_ || (DCT_ != 0 && !MDCT_ && !IMDCT_), "DST: the sign and the reversal on a plain DCT tile");
    // CONV (with R2C): y = irfft(rfft(x, 2N) . G, 2N)[o .. o + Lo) of real rows, the FFT convolution (or, with the conjugate of
    // G, correlation) in ONE tile: load, passes, product, the same passes again, store.  The load packs a row of L <= 2N reals
    // as the R2C rows are packed, with zeros from sample L on (pair loads inside the row, real by real at its end: L may be
    // odd).  After the passes the work item of the pair (k, N - k) unpacks X[k] and X[N-k] as the R2C store does, multiplies
    // them by G[d][k] and G[d][N-k] -- two runs over the lanes from global memory, d = the row's global index modulo D --
    // folds the products with the C2R load's algebra (the imaginary parts of bins 0 and N dropped, as numpy's irfft drops
    // them) and writes conj Z back to the two slots it read: it is their only reader.  A row tile's pass 0 gathers from the
    // layout its last pass scatters to -- lds_index<C, -1> and lds_index<C, NP - 1> are both the unswizzled row -- so after
    // one barrier run_pass runs a second time on the same tables and register twiddles and leaves conj(z) of the packed
    // result; no second layout exists that another work item could still be reading.  The store scales by 1 / 2N, negates
    // the odd samples' conjugation away and writes sample t of a row to out[r Lo + t - o] for o <= t < o + Lo only, each
    // exactly once: a pair whose two samples are both wanted and whose address is aligned to two elements goes out as one
    // access, every other wanted sample as one real.  x is read once, y written once; G is re-read by every row through
    // L2 and the Infinity Cache.  No LDS beyond the R2C tile's.  A row's result depends on its own data and filter row alone.
    static constexpr bool CONV = CONV_;
    static_assert(!CONV_ || (R2C_ && !FIRST_DIRECT_ && DCT_ == 0 && !STFT_ && SPEC_ == 0 && NT_ == 0 && R0_ <= 32 && R1_ <= 32 &&
                             (same_t<IT_, T_>::value ||
                              (same_t<T_, float>::value && (same_t<IT_, _Float16>::value || same_t<IT_, bf16_t>::value)))),
                  "CONV: packed real rows of the plan's own float type, or of a 16-bit float under float, staged in LDS by the "
                  "zero-extending load");
    // The STORAGE type of a CONV tile is IT: x, both gates and the result (WGRAD: x, gy and both gates) are arrays of IT, widened exactly
    // in the loads and rounded once, to nearest even, in the stores (sload / sstore above).  The filter spectra, the tables,
    // the LDS tile, the accumulators and WGRAD's result stay T.
    // OLS (with CONV): overlap-save.  A signal row of T samples is convolved as F blocks of 2N samples, each one launch row
    // and one CONV tile row: block f loads the samples s0 + f S .. s0 + f S + 2N - 1 of its signal (zeros outside the row,
    // never loaded; one pair load where both samples lie inside, as aligned as the block's start), and of its circular result
    // stores the S samples from c on -- those no wrap-around touched, by the caller's choice of c and S -- to out[f S ..] of
    // the signal's row of Lo samples, the last block up to Lo.  Every output sample is written exactly once by exactly one
    // block: no overlap-add, no carry between tiles, no scratch.  Tiles may straddle signals: (signal, block) of the tile's
    // first row is computed once, uniformly, and wrapped per row as the STFT load wraps its frames.  The filter row follows
    // the signal, not the launch row.  The passes, the product and the fold are CONV's.
    static constexpr bool OLS = OLS_;
    static_assert(!OLS_ || CONV_, "OLS: the overlap-save twin of a CONV tile");
    // GATE (with CONV): bit 0 the pregate, y = conv(a . x): every sample the load reads is multiplied by the element of
    // TileParams::gate_in at the same (signal row, sample) before it goes to LDS -- one multiply in T; a position the load
    // zero-extends reads no gate.  Bit 1 the postgate, y = b . conv(x): the finished sample v * scale (signed as ever) is
    // multiplied by the element of TileParams::gate_out at the same (signal row, sample) immediately before the store -- a
    // multiplication of its own, never folded into the scale, so that the result equals the ungated kernel's on a . x, times
    // b, bit for bit.  A gate is read in pairs (gload_pair: aligned to one element) exactly where x is read, or the result
    // stored, in pairs, and real by real elsewhere; the gate load stands beside the access it accompanies, issued with it.
    static constexpr int GATE = GATE_;
    static_assert(GATE_ >= 0 && GATE_ <= 3 && (GATE_ == 0 || CONV_), "GATE: the pregate (1) and postgate (2) of a CONV tile");
    // WGRAD (with CONV, any GATE, never PART): the filter gradient of the convolution, gk[d][j] = sum over the rows r of channel d and the
    // samples t of gy[r][t] x[r][t - j], as the sum over PAIRS (signal row r, block f) of conj(U) G, U and G the half spectra
    // of the u-block the forward block loaded (CONV's / OLS's load) and of the g-block -- the part of gy the forward block
    // stored, put back where the block had it: gb[i] = gy[r][f S + i - c] for c <= i < c + S, f S + i - c < Lo, zero elsewhere.
    // The exact adjoint of the forward block, circular where that is.  A grid of D P persistent workgroups, workgroup
    // (d, s) walking slice s of the B F pairs of channel d -- contiguous, ascending, lengths differing by one at most -- TILE
    // pairs at a time: load the u-blocks, passes, every work item unpacks the bin pairs (k, N - k) it owns into registers,
    // barrier, the g-blocks into the same LDS, passes, unpack, multiply by the conjugates of the held values and add into
    // register accumulators per (tile row, bin pair).  At the end the TILE rows are summed in ascending order through the
    // tile's own LDS and row (s D + d) of N + 1 bins is stored, unscaled, once (conjugated when the forward correlated).
    // x and gy are read once each; no spectrum of a row reaches memory, no scratch, no atomics; the order of every sum is
    // fixed by the plan, so the result is bit-identical from run to run.  wgrad_walk below; the main tile loop is not run.
    // With GATE the gates of the forward plan are fused into the two block loads, as CONV's pregate is into its load: bit 0,
    // every sample read from x is multiplied by the element of TileParams::wgrad_pregate at the same (signal row, sample);
    // bit 1, every sample read from gy by the element of TileParams::gate_out at the same (signal row, t), gy's coordinates.
    // One multiplication of its own in T (widened first on a 16-bit storage type) before the value goes to LDS; a position
    // a load zero-extends reads no gate.  The bins equal the ungated kernel's on the products a . x and b . gy bit for bit.
    static constexpr bool WGRAD = WGRAD_;
    static_assert(!WGRAD_ || CONV_, "WGRAD: the filter-gradient twin of a CONV / OLS tile");
    // WSPEC (with WGRAD, any GATE): the store variant of the filter-gradient tile, stage 1 of the fused partitioned filter
    // gradient (conv.cpp, lag_corr.hip).  1: the walk runs WGRAD's u-block load alone (zero extension, pregate, widening),
    // 2: its g-block load alone (the band [c, c + S), postgate); then the passes and the unpack of bin pairs as ever, and
    // instead of accumulating every work item STORES the bins it unpacked: block f of signal row r goes to row (r F + f) of
    // `out`, (rows, F, N + 1) complex values of type T, unscaled and unconjugated -- frames-major, whole lines, each value
    // written once.  The slices of a channel's (signal, block) pairs and the grid of D P workgroups are WGRAD's; nothing is
    // summed, so P only spreads the work.  No accumulators, no reduction through LDS.
    static constexpr int WSPEC = WSPEC_;
    static_assert(WSPEC_ >= 0 && WSPEC_ <= 2 && (WSPEC_ == 0 || WGRAD_), "WSPEC: the spectrum-store twin of a WGRAD tile");
    // PART (with CONV and OLS, any GATE): uniformly partitioned overlap-save, for filters longer than half a block.  The filter
    // is P partitions of Q taps with one spectrum each, H[d][p]; output block f of a signal is the sum over p of the spectrum of
    // the n samples from s0 + f S - p Q on (correlation: + p Q) times H[d][p] (its conjugate), folded and inverted ONCE.  A step
    // of the persistent grid takes TILE launch rows (signal, block) as the OLS tile does and, for p = 0 .. P - 1 in ascending
    // order, loads the shifted blocks with the OLS load (pregate included: read again for every partition), runs the passes,
    // unpacks the bin pairs (k, N - k) as the CONV product stage does and adds their products with row (d, p) of the spectra
    // into register accumulators per (tile row, bin pair), laid out as WGRAD's.  A partition in which no row of the tile reads
    // a sample of [0, T) is skipped whole (a uniform test: no load, no passes); a row whose own block is empty loads zeros
    // and its filter loads and products are predicated off, so a row's sum has exactly the terms of its own live partitions,
    // in ascending p, whatever tile it shares: bit-identical for any batch, slab and grid.  Then the C2R fold of the sums,
    // the passes again and the OLS store (postgate included).  No scratch, no atomics, no LDS beyond the tile's; the input
    // spectra are recomputed, never stored, so the work grows with P.  part_walk below; the main tile loop is not run.
    static constexpr bool PART = PART_;
    static_assert(!PART_ || (CONV_ && OLS_ && !WGRAD_ && TILE_ <= 64), "PART: the partitioned twin of an OLS tile");
    // PAIR (with CONV; never OLS, PART, WGRAD or GATE): the second operand is a SIGNAL, one row of its own per row of x, not a
    // filter spectrum: out[r] = irfft(rfft(xe) G, 2N)[o .. o + Lo), xe the 2N samples that hold x[r] (conv_len reals) from
    // index pair_ea on and zeros elsewhere, G = rfft(ve) or its conjugate (conv_mode bit 0), ve holding v[r] (pair_K reals)
    // from pair_eb on.  A step of the persistent grid takes TILE rows as the CONV tile does: the x-rows are loaded with the
    // zero-extending load (packed element m holds the samples 2m - ea and 2m + 1 - ea of its row: a pair load where both lie
    // inside, real by real at the ends, nothing outside), the passes run, every work item unpacks the bin pairs (k, N - k) it
    // owns into registers; the v-rows go through the same LDS, passes and unpack; the products are folded with the C2R algebra
    // into the two slots the item just read, the passes run again and the store writes the samples o .. o + Lo - 1, scaled by
    // 1 / 2N, each exactly once (a pair as one access where both samples are wanted and the address is aligned to two
    // elements).  x and v are read once each -- they may be the same buffer -- and no spectrum reaches memory; no scratch, no
    // atomics, no LDS beyond the R2C tile's, no accumulators.  A row's result depends on that row of x and of v alone.  Rows
    // from the tile's nv live ones on load zeros and store nothing.  pair_walk below; the main tile loop is not run.
    static constexpr bool PAIR = PAIR_;
    static_assert(!PAIR_ || (CONV_ && !OLS_ && !PART_ && !WGRAD_ && GATE_ == 0 && same_t<IT_, T_>::value),
                  "PAIR: the two-signal twin of a plain CONV tile of the plan's own float type");
    // ADJ (with ISTFT): the adjoint of the framed, windowed, one-sided transform instead of its inverse -- the gradient of stft
    // with respect to the signal.  1: `in` is the incoming gradient g = dL/dRe X + i dL/dIm X.  The C2R load doubles the real
    // parts of bins 0 and N (their imaginary parts drop out as they always have), so the passes leave
    // Re sum_{k <= N} g[k] e^(+2 pi i j k / 2N) * 2; the synthesis table carries the 1 / 2 (stft_win = gain * w[j] / 2 with the
    // sign of the conjugation).  The store is the overlap-add without the envelope: istft_env is never read, the sample at
    // padded position u in [cen, cen + stft_len) goes to out[b, u - cen], and with stft_center == 1 (reflect) the samples below
    // cen and the N from cen + stft_len on go to adj_edge[b, 0, u] and adj_edge[b, 1, u - cen - stft_len] for the caller to
    // fold back.  Plain stores, each element once, suppressed in warm-up tiles as the stores to `out` are.
    // 2 / 3: the adjoint of the power / magnitude spectrogram.  `in` is X itself and adj_mult the incoming real gradient m; the
    // load multiplies X[k] by m[k] (2: the factor 2 of d|X|^2 is the table's, stft_win = gain * w[j]) or by m[k] / |X[k]|, zero
    // where |X[k]| is (3), so that the product never exists in memory.
    static constexpr int ADJ = ADJ_;
    static_assert(ADJ_ >= 0 && ADJ_ <= 3 && (ADJ_ == 0 || ISTFT_), "ADJ: the adjoint twin of an ISTFT tile");
    // IADJ (with STFT): the adjoint of the inverse STFT -- the gradient of istft with respect to its frames -- which is the
    // one-sided STFT of gy / envelope.  `in` is the incoming gradient gy, (entries, stft_len) reals; stft_frames is the frame
    // count of X (the plan's payload: `length` may have cropped the signal), stft_center 0 or 2.  The load multiplies the
    // sample at padded position u = frame * hop + j by istft_env[u], the table the inverse plan divides by, when
    // t = u - (centred ? N : 0) lies in [0, stft_len), and SELECTS an exact zero otherwise: neither gy nor the table is read
    // there (the envelope may vanish outside the stored range, gy may hold anything), so a frame that sees no stored sample
    // is an exact zero.  A frame wholly inside its entry loads gy and the table with one paired access each.  stft_win is
    // 2 gain w[j] / 2N; the store halves bins 0 and N (c_0 = c_N = 1, every other c_k = 2) and writes an exact zero into their
    // imaginary parts, which the forward ignores.  No LDS, scratch or atomics beyond the STFT tile's; a frame's result does not
    // depend on batch, slab or grid.
    static constexpr bool IADJ = IADJ_;
    static_assert(!IADJ_ || (STFT_ && SPEC_ == 0 && !CONV_ && !MDCT_), "IADJ: the adjoint load and store of a plain STFT tile");
    // An even N lets one thread move FOUR adjacent reals x[4e .. 4e+3] at once: they are the packed elements
    // z_e = (x[4e], x[4e+2]) and z_(N-1-e) = (x[4e+3], x[4e+1]) -- one 16-byte HBM access and two whole LDS elements instead
    // of two 8-byte accesses and four 4-byte LDS slots (forward 15-25 % faster).  An odd N (n = 30) moves pairs,
    // and so does every N under -DMIFFT_DCT_PAIRS (the A/B of profiles/r06_dct_ab.txt).  The accesses are as aligned as the
    // caller's x and out: to one element at least, which the hardware's unaligned global accesses serve.
#ifdef MIFFT_DCT_PAIRS
    static constexpr bool DCT_QUADS = false;
#else
    static constexpr bool DCT_QUADS = (DCT_ == 2 || DCT_ == 3) && !COLS_ && N_ % 2 == 0;
#endif
    // STFT (torch.stft over real signals): an R2C tile whose rows are the overlapping FRAMES of a signal instead of the rows of
    // a tensor.  Only the load differs: row r = r0 + c of the launch is frame r % F of batch entry r / F, its packed element m
    // the two reals at s = frame * hop - (centred ? N : 0) + 2 m and s + 1 of that entry, times the window's values 2 m and
    // 2 m + 1 (TileParams::stft_*).  A row that lies inside its entry loads every pair with one access, aligned to one element
    // like the DCT rows below; a row that reaches beyond either end (centred plans only) loads real by real with the index
    // reflected (i < 0 -> -i, i > T - 1 -> 2 (T - 1) - i) or replaced by zero.  The choice is per row.  Neighbouring frames
    // re-read the same lines through L2 and the Infinity Cache; nothing outside [0, T) of an entry of the launch is touched.
    // The passes, the unpacking store (one row of N + 1 bins per frame) and the persistent walk are the R2C tile's.
    static constexpr bool STFT = STFT_;
    static_assert(!STFT_ || (R2C_ && !FIRST_DIRECT_ && DCT_ == 0 && same_t<IT_, T_>::value),
                  "STFT: packed real rows of the plan's own float type, staged in LDS by the framing load");
    // ISTFT (torch.istft, real output): a C2R tile whose rows are TILE consecutive FRAMES of ONE batch entry and whose store
    // overlap-adds them.  Load and passes are the C2R tile's (row r of entry b is spectrogram row b F + r); the last pass
    // leaves conj(z) of the packed frames in LDS, unscaled.  The store has one work item per padded sample
    // u in [f0 hop, (f0 + nv - 1) hop + 2 N) of the tile's frames f0 .. f0 + nv - 1: it starts from the partial sum the
    // earlier tiles of the entry left in `carry` (2 N - hop reals behind the tables; exact zero in the first tile of an entry
    // and beyond the carry), adds ws[j] y_f[j], j = u - f hop, for the tile's frames that cover u in ASCENDING f, each term
    // one fma, and either finishes the sample -- u < (f0 + nv) hop, or the tile is the last of its entry: times
    // istft_env[u], stored to out[b, u - c] when that lies in [0, T) -- or leaves it in the carry at u - (f0 + nv) hop.
    // ws (stft_win) is gain * w[j] / 2N with the sign of the conjugation folded in (odd j negative), so a term is one fma
    // on the LDS slot as it stands.  The carry moves towards lower indices: the samples are walked in ascending chunks of
    // THREADS with a barrier between a chunk's reads and its writes.  A workgroup owns one contiguous ascending run of tiles
    // (lengths differ by one at most); a run that starts inside an entry first recomputes the W tiles before it with the
    // stores suppressed (tile_kernel), so every sample is summed in ascending frame order from an exact zero whatever the
    // partition, and the result of an entry does not depend on the grid.  Every output sample is written exactly once, with
    // a plain store; nothing outside [0, T) of an entry of the launch is touched.
    // SPEC (spectrogram: |X| or |X|^2 of an STFT tile, 1 magnitude, 2 power): only the store differs.  The work item of the
    // pair (k, N - k) holds a = X[k] and b = X[N-k]; instead of two complex bins it writes two reals, a.x^2 + a.y^2 (one
    // product and one fma) or its sqrt, into a row of N + 1 reals per frame -- half the bytes, and the complex spectrogram
    // never exists.  Rows of N + 1 reals start at any element, so the stores are aligned to one element.
    // FB (with SPEC): a banded filterbank of spec_bands bands follows in the same launch.  The pair's work item leaves its
    // two reals IN PLACE -- P[k] in .x of slot k for k < N, P[N] in .y of slot 0; it is the only reader of those slots, so
    // no LDS is added and every length that plans as an STFT plans here -- and stores nothing.  After a barrier one work
    // item per (row c < nv, band m), m fastest, sums spec_wt[off[m] + j] * P[c][lo[m] + j] over ascending j, one fma per
    // term from an exact zero, and stores out[(row0 + c) * spec_bands + m]: a row's stores are contiguous, a band without
    // bins stores an exact 0, rows c >= nv store nothing.  The order of summation is fixed per frame, so a frame's result
    // does not depend on batch, slab or grid.  The band tables are read from global memory (TileParams::spec_*): a few
    // hundred bytes that every workgroup re-reads, resident in L2 and the vector L1 after the first tile, whereas a copy
    // in LDS would not fit beside the longest rows, which fill it.  The cost is proportional to the spans of the bands: a
    // dense matrix is correct but slow (no MFMA: a mel filter spans a handful of bins).
    static constexpr int SPEC = SPEC_;
    static constexpr bool FB = FB_;
    static_assert(SPEC_ >= 0 && SPEC_ <= 2 && (SPEC_ == 0 || STFT_) && (!FB_ || SPEC_ != 0),
                  "SPEC: the magnitude / power store of an STFT tile; FB: its filterbank");
    // LOG (with SPEC): every value v the store would write -- a bin without FB, a band with it -- becomes
    // fma(a, log2(max(v + add, amin)), c) first (TileParams::spec_*; the library logarithm, one explicit fma).
    // POST (with FB): a dense (M, Q) matrix follows the bands in the same launch, M <= N - 1.  The band loop stores
    // nothing: y[m] goes to the .y of slot 1 + m of its row, which is dead -- P[k] lives in .x of slot k and P[N] in .y of
    // slot 0, the other .y halves hold stale Z -- so no LDS is added.  The band loop of such a configuration reads only the
    // 4- or 8-byte component it uses, since a neighbour may be writing the other half of the slot.  After a barrier one
    // work item per (row c < nv, q < Q), q fastest, sums post[m * Q + q] * y[c][m] over ascending m, one fma per term from an
    // exact zero, and stores out[(row0 + c) * Q + q]: adjacent lanes read adjacent q of one m from global memory (the
    // matrix is a few KB, re-read from L1 / L2 by every tile as the band tables are) and the same y[m] from LDS, a
    // broadcast.  The order of summation is fixed per frame.
    static constexpr bool LOG = LOG_;
    static constexpr bool POST = POST_;
    static_assert((!LOG_ || SPEC_ != 0) && (!POST_ || FB_), "LOG: the log stage of a SPEC store; POST: the matrix after FB");
    static constexpr bool ISTFT = ISTFT_;
    static_assert(!ISTFT_ || (C2R_ && !LAST_DIRECT_ && DCT_ == 0 && !STFT_ && ROWPAD_ == 0),
                  "ISTFT: folded rows whose last pass stays in LDS for the overlap-add");
    static constexpr int CPITCH = TSTORE_ ? TILE_ + 1 : TILE_;
    static_assert(!TSTORE_ || (COLS_ && !LAST_DIRECT_ && FIRST_DIRECT_), "TSTORE: column tile, last pass left in LDS");
    static constexpr int DATA_ELEMS = COLS_ ? N_ * CPITCH : LD * TILE_;
    // BIGP0: the first radix is a prime too large for a register butterfly (> 32).  Pass 0 then runs cooperatively in
    // LDS (bigprime_pass0): the row is staged by the flat copy, paired into sums / differences in place, and every
    // thread accumulates a few output pairs over the (R-1)/2 pairs with a cos/sin table of R entries kept behind the
    // twiddle table.  Instantiated by the runtime-specialised kernels only.
    static constexpr bool BIGP0 = R0_ > 32;
    // a second prime above 32 is pass 1 (its inputs are twiddled while they are paired)
    static constexpr bool BIGP1 = NP_ > 1 && R1_ > 32;
    static_assert(!(R2_ > 32 || R3_ > 32) && (!BIGP1 || BIGP0), "cooperative passes come first, at most two");
    static constexpr bool BIGP(int i) { return i == 0 ? BIGP0 : i == 1 ? BIGP1 : false; }
    // per cooperative pass: the cos/sin table of R entries (bigprime_pass), or the Rader tables (rader_pass)
    // (RADERM: bit i = cooperative pass i runs as a Rader convolution; chosen by the host -- it pays from R ~ 128 on and
    //  needs LDS for its tables -- and uploaded tables go with it)
    static constexpr bool RADER(int i) { return BIGP(i) && ((RADERM_ >> i) & 1) != 0; }
    static_assert(RADERM_ == 0 || ((!(RADERM_ & 1) || rader_len(R0_) > 0) && (!(RADERM_ & 2) || rader_len(R1_) > 0)),
                  "Rader pass: no convolution length that splits into register butterflies");
    static constexpr int cs_size(int i) {
        return !BIGP(i) ? 0 : RADER(i) ? rader_lds_elems(R(i), TILE_ * NB(i), 2 * (int)sizeof(T_)) : R(i);
    }
    // (data members: evaluated once at compile time -- a runtime call of rader_len factorises thousands of integers)
    static constexpr int CS_SIZE0 = cs_size(0), CS_SIZE1 = cs_size(1);
    static constexpr int CS_OFF(int i) { return i == 0 ? 0 : CS_SIZE0; }
    static constexpr int CS_ELEMS = CS_SIZE0 + CS_SIZE1;
    static_assert(!BIGP0 || (!FIRST_DIRECT_ && TWMODE_ == TW_LDS), "big-prime pass 0: tile staged in LDS first");
    // DMA: the flat HBM -> LDS copy of the NEXT tile runs asynchronously (global_load_lds) into a staging
    // buffer behind the twiddle table while this tile's passes execute
    static constexpr bool DMA = DMA_;
    static constexpr int STAGE_OFF = ((DATA_ELEMS + TWL_TOTAL) * 2 * (int)sizeof(T_) + 15) / 16 * 16 / (2 * (int)sizeof(T_));
    static constexpr int STAGE_ELEMS = DMA_ ? N_ * TILE_ : 0;
    // HERM: one column of N results carried from a tile to the next one of the workgroup's run (see the HERM stores)
    // (full-line tiles only: narrower ones need the XCD_CHUNK order above -- their neighbours have to run at the same time
    //  on one XCD, or every line is fetched once per tile that shares it: 2- and 4-column tiles 1.2-1.6x slower in runs)
    static constexpr bool HERM_RUNS = HERM_ && !XCD_CHUNK;
    static constexpr int HERM_OFF = DATA_ELEMS + TWL_TOTAL + CS_ELEMS;
    static constexpr int HERM_ELEMS = HERM_RUNS ? N_ : 0;
    // ISTFT: the carry, 2 N - hop <= 2 N reals, where the Hermitian column would be (C2R excludes HERM)
    static constexpr int ISTFT_OFF = HERM_OFF;
    static constexpr int ISTFT_ELEMS = ISTFT_ ? N_ : 0;
    // IMDCT: the carry, v[0 .. N) of a tile's last frame: N reals (DCT = 4 excludes HERM and ISTFT)
    static constexpr int IMDCT_OFF = HERM_OFF;
    static constexpr int IMDCT_ELEMS = IMDCT_ ? (N_ + 1) / 2 : 0;
    static_assert(!(HERM_ && DMA_), "HERM: no staging buffer");
    static constexpr size_t LDS_BYTES =
        DMA_ ? (size_t)(STAGE_OFF + STAGE_ELEMS) * 2 * sizeof(T_)
             : (size_t)(DATA_ELEMS + TWL_TOTAL + CS_ELEMS + HERM_ELEMS + ISTFT_ELEMS + IMDCT_ELEMS) * 2 * sizeof(T_);
    static_assert(P(NP_) == N_, "radices must multiply to N");
    static_assert(LDS_BYTES <= 160 * 1024, "tile + twiddle table exceed the CU's 160 KiB of LDS");
};

// XOR swizzle of the in-row index for the exchange written by pass E (power-of-two rows
// only): the 16 lanes of a ds_write_b64 group own 16 butterflies whose outputs are P*R
// elements apart; fold the low butterfly bits into the bank-selecting low 4 index bits.
template <class C, int E>
MIFFT_DEV int swz(int n) {
    if constexpr (!C::COLS && is_pow2_ce(C::N) && E >= 0 && E < C::NP - 1) {
        // LG = log2(lanes per ds_write group): 16 for 8-byte elements (b64), 8 for 16-byte (b128)
        constexpr int LG = sizeof(typename C::T) == 4 ? 4 : 3;
        constexpr int a = ilog2_ce(C::P(E)), c = ilog2_ce(C::P(E) * C::R(E));
        constexpr int c4 = c < LG ? c : LG, hi = c > LG ? c : LG, nb = c4 - a;
        if constexpr (nb > 0 && (1 << hi) < C::N) {
            return n ^ (((n >> hi) & ((1 << nb) - 1)) << a);
        } else {
            return n;
        }
    } else {
        return n;
    }
}

template <class C, int E>
MIFFT_DEV int lds_index(int c, int n) {
    if constexpr (C::COLS)
        return n * C::CPITCH + c;
    else
        return c * C::LD + swz<C, E>(n);
}

// paired-column DCT tiles: element j of Makhoul's sequence v is row 2j of the column (j < ceil(N / 2)) or row 2 (N-1-j) + 1;
// and its inverse, the element a row goes to
template <class C>
MIFFT_DEV int dct_row_of(int j) {
    return j < (C::N + 1) / 2 ? 2 * j : 2 * (C::N - 1 - j) + 1;
}
template <class C>
MIFFT_DEV int dct_elem_of(int row) {
    return (row & 1) ? C::N - 1 - (row >> 1) : row >> 1;
}

template <class C>
MIFFT_DEV long long gaddr(const TileParams& p, long long base, int c, int n) {
    if constexpr (C::COLS)
        return base + (long long)n * p.inner + c;
    else
        return base + (long long)c * C::N + n;
}

// Addressing split for HBM accesses: address = (uniform tile pointer + uniform element step) + 32-bit lane
// offset.  The uniform part lives in SGPRs, each butterfly carries ONE offset VGPR for all of its R accesses
// (global_load v, v_off, s[base] form) instead of R 64-bit address pairs.
template <class C>
MIFFT_DEV unsigned lane_off(const TileParams& p, int c, int n) {  // n: element index inside the transform
    if constexpr (C::COLS)
        return (unsigned)n * (unsigned)p.inner + (unsigned)c;
    else
        return (unsigned)c * (unsigned)C::N + (unsigned)n;
}
template <class C>
MIFFT_DEV long long elem_stride(const TileParams& p) {
    if constexpr (C::COLS)
        return p.inner;
    else
        return 1;
}

template <class C, int I>
MIFFT_DEV void item_decode(int id, int& c, int& b) {
    if constexpr (C::COLS) {
        b = id / C::TILE;
        c = id - b * C::TILE;
    } else {
        c = id / C::NB(I);
        b = id - c * C::NB(I);
    }
}

// work item k of thread tid in pass I -> (transform c of the tile, butterfly b); false: no such item
template <class C, int I>
MIFFT_DEV bool item_of(int tid, int k, int& c, int& b) {
    if constexpr (C::WSUB && I >= 1) {
        const int wave = tid >> 6, lane = tid & 63;
        const int m = k * C::WSLOTS + lane / C::TILE;  // pair (local sub-problem, butterfly inside it)
        c = lane % C::TILE;
        const int pl = m % C::SPW, qq = m / C::SPW;
        b = qq * C::R(0) + wave * C::SPW + pl;  // b mod R0 = the sub-problem
        return (C::WPER(I) % C::WSLOTS == 0) || m < C::WPER(I);
    } else {
        const int id = tid + k * C::THREADS;
        item_decode<C, I>(id, c, b);
        return (C::ITEMS(I) % C::THREADS == 0) || id < C::ITEMS(I);
    }
}

// order one wave's LDS accesses across a pass boundary for the COMPILER (the hardware executes one wave's LDS
// instructions in order; there is nothing to wait for)
// every vector-memory operation of this wave issued so far is complete (s_waitcnt vmcnt(0), visible to the compiler's
// own wait-count bookkeeping) and nothing scheduled after it moves above
MIFFT_DEV void vm_drain() {
    __builtin_amdgcn_s_waitcnt(0x0F70);  // gfx9 encoding: vmcnt = 0, expcnt / lgkmcnt unconstrained
    __builtin_amdgcn_sched_barrier(0);
}

MIFFT_DEV void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// flat offset f of a row tile's footprint -> (transform c of the tile, element n): rows f = c N + n; ILV blocks
// f = g N I + n I + ci with c = g I + ci (constant divisors)
template <class C>
MIFFT_DEV void ilv_decode(int f, int& c, int& n) {
    if constexpr (C::ILV > 0) {
        constexpr int I = C::ILV;
        const int g = f / (C::N * I), r = f - g * (C::N * I);
        n = r / I;
        c = g * I + (r - n * I);
    } else {
        c = f / C::N;
        n = f - c * C::N;
    }
}

// ILV: the flat copies of the tile's run of `total` elements, in chunks of up to 16 elements per thread whose HBM accesses
// are all issued before the first LDS access (a load-then-write loop keeps one load in flight per wave: 12-25 % of HBM
// bandwidth).  Loads past the end of a ragged last tile re-read its last element (branch-free; never stored).
template <class C>
MIFFT_DEV void ilv_load(const TileParams& p, cpx<typename C::T>* lds, long long base, int total, int tid) {
    using T = typename C::T;
    using V = cpx<T>;
    constexpr int IT = (C::TILE * C::N + C::THREADS - 1) / C::THREADS, CH = IT < 16 ? IT : 16;
#pragma unroll 1
    for (int k0 = 0; k0 < IT; k0 += CH) {
        V x[CH];
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            int f = tid + (k0 + j) * C::THREADS;
            f = f < total ? f : total - 1;
            if constexpr (!same_t<typename C::IT, T>::value)
                x[j] = load_foreign<C>(p.in, base + f);
            else if constexpr (C::IN_REAL)
                x[j] = {gload_real<(C::NT & 1) != 0>((const T*)p.in + base + f), (T)0};
            else
                x[j] = gload<(C::NT & 1) != 0>((const V*)p.in + base + f);
        }
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            const int f = tid + (k0 + j) * C::THREADS;
            if ((IT % CH == 0 || k0 + j < IT) && f < total) {
                int c, n;
                ilv_decode<C>(f, c, n);
                V v = x[j];
                if (p.inverse && C::CONJ_IN) v.y = -v.y;
                lds[lds_index<C, -1>(c, n)] = v;
            }
        }
    }
}
template <class C>
MIFFT_DEV void ilv_store(const TileParams& p, const cpx<typename C::T>* lds, long long base, int total, int tid) {
    using T = typename C::T;
    using V = cpx<T>;
    constexpr int IT = (C::TILE * C::N + C::THREADS - 1) / C::THREADS, CH = IT < 16 ? IT : 16;
    V* gout = (V*)p.out;
#pragma unroll 1
    for (int k0 = 0; k0 < IT; k0 += CH) {
        V y[CH];
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            int f = tid + (k0 + j) * C::THREADS, c, n;
            f = f < total ? f : total - 1;
            ilv_decode<C>(f, c, n);
            y[j] = lds[lds_index<C, C::NP - 1>(c, n)];
        }
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            const int f = tid + (k0 + j) * C::THREADS;
            if ((IT % CH == 0 || k0 + j < IT) && f < total) {
                V v = y[j];
                if (p.inverse) {
                    v.x *= (T)p.scale;
                    v.y *= -(T)p.scale;
                }
                gstore<(C::NT & 2) != 0>(gout + base + f, v);
            }
        }
    }
}

// FS1: tile t = (outer o, n2, column tile): load base / store base / twiddle row n2
template <class C>
MIFFT_DEV void tile_geom_fs1(const TileParams& p, long long t, long long& base, long long& obase, int& nv, int& n2) {
    const long long tiles_per_row = (p.fs_inner + C::TILE - 1) / C::TILE;
    const long long o = t / p.tiles_per_outer, r = t - o * p.tiles_per_outer;
    const long long row = r / tiles_per_row, c0 = (r - row * tiles_per_row) * C::TILE;
    const long long left = p.fs_inner - c0;
    nv = (int)(left < C::TILE ? left : C::TILE);
    n2 = (int)row;
    const long long image = o * (long long)C::N * p.inner;  // N1 * (N2 * fs_inner) elements per outer index
    base = image + row * p.fs_inner + c0;
    obase = image + row * (long long)C::N * p.fs_inner + c0;
}

template <class C>
MIFFT_DEV void tile_geom(const TileParams& p, long long t, long long& base, int& nv) {
    if constexpr (C::FS1) {
        long long obase;
        int n2;
        tile_geom_fs1<C>(p, t, base, obase, nv, n2);
    } else if constexpr (C::COLS) {
        const long long o = t / p.tiles_per_outer;
        const long long c0 = (t - o * p.tiles_per_outer) * C::TILE;
        const long long left = (p.col_lim ? p.col_lim : p.inner) - c0;
        nv = (int)(left < C::TILE ? left : C::TILE);
        base = o * (long long)C::N * p.inner + c0;
    } else {
        const long long r0 = t * C::TILE;
        const long long left = p.n_rows - r0;
        nv = (int)(left < C::TILE ? left : C::TILE);
        base = r0 * C::N;
    }
}

template <class C, int I>
MIFFT_DEV void preload_tw(cpx<typename C::T>* twr, const cpx<typename C::T>* tw, int tid, int inverse) {
    if constexpr (I < C::NP) {
        constexpr int R = C::R(I), P = C::P(I), RATIO = C::N / (P * R);
#pragma unroll
        for (int k = 0; k < C::IPT(I); ++k) {
            int id = tid + k * C::THREADS, c, b;
            if (id >= C::ITEMS(I)) id = 0;
            item_decode<C, I>(id, c, b);
            const int pp = b % P;
#pragma unroll
            for (int j = 1; j < R; ++j) {
                cpx<typename C::T> w = tw[j * pp * RATIO];
                if (inverse) w.y = -w.y;  // plan table is conjugated for inverse plans; we need W forward
                twr[C::TW_OFF(I) + k * (R - 1) + (j - 1)] = w;
            }
        }
        preload_tw<C, I + 1>(twr, tw, tid, inverse);
    }
}

template <class C, int I>
MIFFT_DEV void fill_lds_tw(cpx<typename C::T>* ltw, const cpx<typename C::T>* tw, int tid, int inverse) {
    if constexpr (I < C::NP) {
        constexpr int R = C::R(I), P = C::P(I), RATIO = C::N / (P * R);
        for (int e = tid; e < P * (R - 1); e += C::THREADS) {
            const int j = e / P + 1, pp = e - (j - 1) * P;
            cpx<typename C::T> w = tw[j * pp * RATIO];
            if (inverse) w.y = -w.y;
            ltw[C::TWL_OFF(I) + e] = w;
        }
        fill_lds_tw<C, I + 1>(ltw, tw, tid, inverse);
    }
}

// Experiment switch: keep the butterflies of one thread apart in the instruction schedule (lower register pressure,
// less ILP).  Off in the product build.
#ifdef MIFFT_SCHED_FENCE
#define MIFFT_FENCE() __builtin_amdgcn_sched_barrier(0)
#else
#define MIFFT_FENCE() ((void)0)
#endif

// In-kernel phase stamps -- DIAGNOSTIC BUILDS ONLY (tools/tune, -DMIFFT_STAMPS; no product kernel executes one).
// Thread 0 of every workgroup accumulates s_memtime deltas per phase in 17 LDS words BEHIND the kernel's dynamic LDS
// (the tuner launches with 256 extra bytes) and copies them to the buffer passed in TileParams::tcol at the end
// ([workgroup][16] shader cycles); stamp values never reach an output element.
#ifdef MIFFT_STAMPS
#ifndef MIFFT_STAMP_TID
#define MIFFT_STAMP_TID 0  // the stamping thread (its wave is the one measured)
#endif
MIFFT_DEV void mifft_stamp(int i, unsigned lds_off, const void* dump = nullptr) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_stamp[];  // the kernel's dynamic LDS
    if (threadIdx.x == MIFFT_STAMP_TID) {
        unsigned long long* a = (unsigned long long*)(smem_stamp + ((lds_off + 15) / 16) * 16);
        const unsigned long long t = __builtin_amdgcn_s_memtime();
        if (i < 0) {
            for (int k = 0; k < 16; ++k) a[k] = 0;
        } else if (i < 16) {
            a[i] += t - a[16];
        } else {
            for (int k = 0; k < 16; ++k) ((unsigned long long*)dump)[(size_t)blockIdx.x * 16 + k] = a[k];
        }
        a[16] = __builtin_amdgcn_s_memtime();
    }
}
#define MIFFT_STAMP(C_, i) mifft_stamp(i, (unsigned)C_::LDS_BYTES)
#define MIFFT_STAMP_DUMP(C_, p_) mifft_stamp(99, (unsigned)C_::LDS_BYTES, (p_).tcol)
#else
#define MIFFT_STAMP(C_, i) ((void)0)
#define MIFFT_STAMP_DUMP(C_, p_) ((void)0)
#endif

// gather the pass-0 inputs of tile (base, nv) from HBM into registers; slice PART of NPARTS: the elements e = k R + j
// with e % NPARTS == PART (NPARTS = 1: all of them)
template <class C, int PART = 0, int NPARTS = 1>
MIFFT_DEV void load_pass0(const TileParams& p, cpx<typename C::T> (*v)[C::R(0)], long long base, int nv, int tid) {
    using T = typename C::T;
    using V = cpx<T>;
    constexpr int R = C::R(0), NB = C::NB(0), IPT = C::IPT(0);
    constexpr bool EXACT = C::ITEMS(0) % C::THREADS == 0;
    const V* gin = (const V*)p.in;
#pragma unroll
    for (int k = 0; k < IPT; ++k) {
        const int id = tid + k * C::THREADS;
        if (EXACT || id < C::ITEMS(0)) {
            int c, b;
            item_decode<C, 0>(id, c, b);
            // No predicate on the loads: a slot beyond the ragged end of the last tile re-reads the last valid
            // transform (always in bounds; its results are never stored).  Branch-free loads stay back to back
            // with a single wait at first use -- per-load exec-masked blocks cost 40 % on the column tiles.
            const int cc = c < nv ? c : nv - 1;
            const unsigned off = lane_off<C>(p, cc, b);
            const long long step = (long long)NB * elem_stride<C>(p);  // uniform: element j sits j*step further
#pragma unroll
            for (int j = 0; j < R; ++j) {
                if ((k * R + j) % NPARTS != PART) continue;  // (compile-time after unrolling)
                if constexpr (!same_t<typename C::IT, T>::value) {
                    v[k][j] = load_foreign<C>(p.in, base + j * step + off);
                } else if constexpr (C::IN_REAL) {
                    v[k][j].x = gload_real<(C::NT & 1) != 0>((const T*)p.in + base + j * step + off);
                    v[k][j].y = (T)0;
                } else if constexpr (C::DCT == 2 && C::COLS) {  // the permuted row: no longer affine in j
                    v[k][j] = gload<(C::NT & 1) != 0>(gin + base + lane_off<C>(p, cc, dct_row_of<C>(b + j * NB)));
                    if constexpr (C::DST) {  // (-1)^row: the odd rows are the elements of the second half of v
                        if (b + j * NB >= (C::N + 1) / 2) v[k][j] = {-v[k][j].x, -v[k][j].y};
                    }
                } else {
                    v[k][j] = gload<(C::NT & 1) != 0>(gin + base + j * step + off);
                }
            }
        }
    }
}

// workgroup barrier.  Kernels with an LDS-DMA in flight (C::DMA) must not use __syncthreads(): its fence
// drains vmcnt and with it the asynchronous copy (cdna_hip_programming.md, "Pipelining across barriers").
template <class C>
MIFFT_DEV void wg_barrier() {
#ifdef MIFFT_ABLATE_BARRIERS  // timing experiment only (results are wrong): what do the workgroup barriers cost?
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    return;
#endif
    if constexpr (C::DMA)
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    else
        __syncthreads();
}

// LDS -> registers: the R inputs of every butterfly this thread owns in pass I, twiddled
template <class C, int I>
MIFFT_DEV void pass_gather_lds(const TileParams& p, const cpx<typename C::T>* src, const cpx<typename C::T>* ltw,
                               const cpx<typename C::T>* twr, cpx<typename C::T> (*v)[C::R(I)], int tid) {
    using T = typename C::T;
    using V = cpx<T>;
    constexpr int R = C::R(I), P = C::P(I), NB = C::NB(I), IPT = C::IPT(I), RATIO = C::N / (P * R);
#pragma unroll
    for (int k = 0; k < IPT; ++k) {
        int c, b;
        if (item_of<C, I>(tid, k, c, b)) {
#pragma unroll
            for (int j = 0; j < R; ++j) v[k][j] = src[lds_index<C, I - 1>(c, b + j * NB)];
            if constexpr (I > 0) {
                const int pp = b % P;
#pragma unroll
                for (int j = 1; j < R; ++j) {
                    V w;
                    if constexpr (C::TWMODE == TW_REG) {
                        w = twr[C::TW_OFF(I) + k * (R - 1) + (j - 1)];
                    } else if constexpr (C::TWMODE == TW_LDS) {
                        w = ltw[C::TWL_OFF(I) + (j - 1) * P + pp];
                    } else {
                        w = ((const V*)p.tw)[j * pp * RATIO];
                        if (p.inverse) w.y = -w.y;
                    }
#ifndef MIFFT_ABLATE_MATH
                    v[k][j] = cmul(v[k][j], w);
#else
                    v[k][j].x += w.x;
#endif
                }
            }
        }
        MIFFT_FENCE();
    }
}

// HERM: the flat column (kz, ky, kx) of the trailing dimensions (herm_d0 x herm_d1 x herm_d2) mirrors to (-kz, -ky, -kx)
MIFFT_DEV int herm_mirror(const TileParams& p, int cf) {
    const int d2 = p.herm_d2, d1 = p.herm_d1;
    const int r = cf / d2, kx = cf - r * d2, kz = r / d1, ky = r - kz * d1;
    return ((kz ? p.herm_d0 - kz : 0) * d1 + (ky ? d1 - ky : 0)) * d2 + (kx ? d2 - kx : 0);
}

// HERM: does this pass compute column cf itself (`own`), and has the column a mirror image other than itself (`twice`)?
// Below the middle of the half axis: yes; beyond it: no (the mirror image's tile stores it); on a self-mirrored index of the
// half axis the flat order of the pair decides.
MIFFT_DEV void herm_owner(const TileParams& p, int cf, int mf, bool& own, bool& twice) {
    const int in_row = cf % p.herm_L, kj = in_row / p.herm_js;
    own = (kj == 0 || 2 * kj == p.herm_dj) ? cf <= mf : 2 * kj < p.herm_dj;
    twice = own && cf != mf;
}
MIFFT_DEV bool herm_twice(const TileParams& p, int cf) {
    bool own, twice;
    herm_owner(p, cf, herm_mirror(p, cf), own, twice);
    return twice;
}
// HERM: tile t -> (outer index, row of the column space, tile inside the covered part of the row)
template <class C>
MIFFT_DEV void tile_geom_herm(const TileParams& p, long long t, long long& base, int& nv, int& col0, int& in_row) {
    const long long o = t / p.tiles_per_outer;
    const int in_image = (int)(t - o * p.tiles_per_outer);
    const int r = in_image / p.herm_tpr;
    in_row = in_image - r * p.herm_tpr;
    col0 = r * p.herm_L + in_row * C::TILE;
    const int left = p.herm_H - in_row * C::TILE;
    nv = left < C::TILE ? left : C::TILE;
    base = o * (long long)C::N * p.inner + col0;
}

// registers -> butterflies -> Stockham scatter (LDS, or HBM for the last pass)
template <class C, int I>
MIFFT_DEV void pass_compute_scatter(const TileParams& p, cpx<typename C::T>* lds, cpx<typename C::T> (*v)[C::R(I)],
                                    long long base, int nv, int tid, long long obase = 0, int fs_row = 0) {
    using T = typename C::T;
    using V = cpx<T>;
    constexpr int R = C::R(I), P = C::P(I), IPT = C::IPT(I);
    constexpr bool DST_GLOBAL = (I == C::NP - 1) && C::LAST_DIRECT;
    V* gout = (V*)p.out;
#pragma unroll
    for (int k = 0; k < IPT; ++k) {
        int c, b;
        if (item_of<C, I>(tid, k, c, b)) {
            const int q = b / P, pp = b - q * P;
            const int o0 = q * P * R + pp;
            // large odd primes scatter every conjugate pair to LDS the moment it is computed (DftOddPrime::run_emit): the
            // R outputs never exist in registers beside the R - 1 sums
            if constexpr (!DST_GLOBAL && is_prime_ce(R) && R >= MIFFT_EMIT_PRIME_MIN) {
                auto emit = [&](int s, V y) { lds[lds_index<C, I>(c, o0 + s * P)] = y; };
                DftOddPrime<R, T, 1>::run_emit(v[k], emit);
                MIFFT_FENCE();
                continue;
            }
#ifndef MIFFT_ABLATE_MATH  // timing experiment only: data movement without butterflies / twiddles
            Dft<R, T, 1>::run(v[k]);
#endif
            if constexpr (DST_GLOBAL && C::FS1) {
                if (c < nv) {
                    // row k1 = o0 + s * P of this tile becomes row n2 * N1 + k1 of the other buffer, times W^(k1 * n2)
                    const unsigned off = (unsigned)o0 * (unsigned)p.fs_inner + (unsigned)c;
                    const long long step = (long long)P * p.fs_inner;  // uniform
                    const V* wtab = (const V*)p.tlo;                    // W_(N1 N2)^m, m < N1 * N2
#pragma unroll
                    for (int s = 0; s < R; ++s) {
                        V w = wtab[(o0 + s * P) * fs_row];
                        if (p.inverse) w.y = -w.y;  // the plan's table is conjugated for inverse plans; forward W here
                        V y = cmul(v[k][s], w);
                        if (p.inverse) {
                            y.x *= (T)p.scale;
                            y.y *= -(T)p.scale;
                        }
                        gstore<(C::NT & 2) != 0>(gout + obase + s * step + off, y);
                    }
                }
            } else if constexpr (DST_GLOBAL && C::HERM) {
                // Every result goes to (k, cf) and, conjugated, to the mirrored point (-k, mf).  The mirror image of an
                // aligned run of TILE columns [c0, c0 + TILE) is the run [m - TILE + 1, m], which starts ONE element past a
                // line boundary: stored as it stands, every mirrored line would be written by two tiles in two pieces
                // (15 + 1 elements for 16-column tiles), each store instruction touching twice the lines -- measured 13-15 %
                // of the whole transform (DESIGN_EXPERIMENTS.md R3.6).  So a workgroup walks a CONTIGUOUS run of tiles in
                // DESCENDING column order and the lane of a tile's first column does not store its own mirror image: it
                // keeps the column in LDS (`carry`, N elements) and stores the column the previous tile kept, which is the
                // missing first element of this tile's mirrored lines.  Only the ends of a run store single elements.
                //   obase = the image's base (outer index); fs_row = the tile's first flat column (bits 0..29),
                //   bit 30: the previous tile of the run left its first column in `carry`, bit 31: leave this tile's there
                const int col0 = fs_row & 0x3fffffff;
                const bool carry_in = (fs_row >> 30) & 1, carry_out = ((unsigned)fs_row >> 31) != 0;
                const int cf = col0 + c, mf = herm_mirror(p, cf);
                bool own, has_mirror;
                herm_owner(p, cf, mf, own, has_mirror);
                const bool alive = c < nv && own;  // (the other columns belong to their mirror image's tile)
                const bool first = c == 0, twice = c < nv && has_mirror;
                const bool keep = first && twice && carry_out;              // first column: left in LDS for the next tile,
                const bool lone = first && twice && !carry_out && carry_in;  // or stored by itself at the end of a run
                const bool mirrored = first ? carry_in || (twice && !carry_out) : twice;           // the mirrored store ...
                const int mcol = first && carry_in ? herm_mirror(p, col0 + C::TILE) : mf;  // ... and its column
                V* carry = lds + C::HERM_OFF;
                const unsigned off = lane_off<C>(p, c, o0);
                const long long step = (long long)P * elem_stride<C>(p);  // uniform
#pragma unroll
                for (int s = 0; s < R; ++s) {
                    V y = v[k][s];
                    if (p.inverse) {
                        y.x *= (T)p.scale;
                        y.y *= -(T)p.scale;
                    }
                    if (alive) gstore<(C::NT & 2) != 0>(gout + base + s * step + off, y);
                    const int kk = o0 + s * P, kr = kk ? C::N - kk : 0;
                    V* const mrow = gout + obase + (long long)kr * p.inner;
                    V z = y;
                    // (the thread that reads carry[kk] here is the one that wrote it in the previous tile: no barrier)
                    if constexpr (C::HERM_RUNS) {
                        if (first && carry_in) z = carry[kk];
                        if (keep) carry[kk] = y;
                    }
                    if (lone) {
                        V w = y;
                        w.y = -w.y;
                        gstore<(C::NT & 2) != 0>(mrow + mf, w);
                    }
                    z.y = -z.y;
                    if (mirrored) gstore<(C::NT & 2) != 0>(mrow + mcol, z);
                }
            } else if constexpr (DST_GLOBAL) {
                if (c < nv) {
                    const unsigned off = lane_off<C>(p, c, o0);
                    const long long step = (long long)P * elem_stride<C>(p);  // uniform
#pragma unroll
                    for (int s = 0; s < R; ++s) {
                        // (HS: store_lim is N / 2 and this is the last pass, o0 < P -- outputs s * P > N / 2 are never stored: a
                        //  compile-time test per unrolled s, so the butterfly's unused results are not even computed)
                        if (C::HS && s * P > C::N / 2) continue;
                        V y = v[k][s];
                        if (p.inverse) {
                            y.x *= (T)p.scale;
                            y.y *= -(T)p.scale;
                        }
                        if constexpr (C::DCT == 3 && C::COLS) {  // element o0 + s P of v: its row of the column
                            if constexpr (C::DST) {  // (an odd row: the second half of v)
                                if (o0 + s * P >= (C::N + 1) / 2) y = {-y.x, -y.y};
                            }
                            gstore<(C::NT & 2) != 0>(gout + base + lane_off<C>(p, c, dct_row_of<C>(o0 + s * P)), y);
                        } else if (!C::HS || o0 + s * P <= p.store_lim)
                            gstore<(C::NT & 2) != 0>(gout + base + s * step + off, y);
                    }
                }
            } else {
#pragma unroll
                for (int s = 0; s < R; ++s) lds[lds_index<C, I>(c, o0 + s * P)] = v[k][s];
            }
        }
        MIFFT_FENCE();
    }
}

// A pass with a prime radix R > 32 (C::BIGP(I)), cooperatively in LDS.  The tile is in LDS (pass 0: staged by the copy).
//   1. in place: a_j = x_j + x_{R-j} at position j, b_j = x_j - x_{R-j} at position R-j   (j = 1..H, H = (R-1)/2)
//   2. per output pair s = 0..H (four consecutive s per thread):  A = x_0 + sum_j cos(2 pi j s / R) a_j,  B = sum_j sin(2 pi j s / R) b_j
//      X_s = A - iB, X_{R-s} = A + iB  -- the conjugate-pair form of DftOddPrime, 4 real FMAs per (j, pair) instead of
//      the 8 of the literal stage (fft/fft/_fft.mojo:261-290); lanes that share a butterfly read a_j, b_j as broadcasts
//   3. after a barrier the outputs go to their Stockham positions
//   (pass I >= 1: the inputs x_j are first multiplied by their Stockham twiddles W_{P R}^{j p} from the LDS table, and
//    the outputs go to q*P*R + p + s*P)
template <class C, int I>
MIFFT_DEV void bigprime_pass(cpx<typename C::T>* lds, const cpx<typename C::T>* ltw, const cpx<typename C::T>* cs, int tid) {
    using T = typename C::T;
    using V = cpx<T>;
    constexpr int R = C::R(I), H = (R - 1) / 2, NB = C::NB(I), P = C::P(I);
    constexpr int PAIRS = C::TILE * NB * H;
    for (int e = tid; e < PAIRS; e += C::THREADS) {
        const int c = e / (NB * H), rem = e - c * (NB * H);
        const int b = rem / H, j = rem - b * H + 1;
        const int i1 = lds_index<C, I - 1>(c, b + j * NB), i2 = lds_index<C, I - 1>(c, b + (R - j) * NB);
        V u = lds[i1], v = lds[i2];
        if constexpr (I > 0) {
            const int pp = b % P;
            u = cmul(u, ltw[C::TWL_OFF(I) + (j - 1) * P + pp]);
            v = cmul(v, ltw[C::TWL_OFF(I) + (R - j - 1) * P + pp]);
        }
        lds[i1] = u + v;
        lds[i2] = u - v;
    }
    __syncthreads();
    // item = (transform, butterfly, group of SB consecutive s): a_j and b_j are read once per j for SB output pairs
    constexpr int SB = MIFFT_BIGP_SB, GROUPS = (H + 1 + SB - 1) / SB;
    constexpr int ITEMS = C::TILE * NB * GROUPS;
    constexpr int IPT = (ITEMS + C::THREADS - 1) / C::THREADS;
    V lo[IPT][SB], hi[IPT][SB];
#pragma unroll
    for (int k = 0; k < IPT; ++k) {
        const int id = tid + k * C::THREADS;
        if (id < ITEMS) {
            const int cb = id / GROUPS, s0 = (id - cb * GROUPS) * SB;
            const int c = cb / NB, b = cb - c * NB;
            const V x0 = lds[lds_index<C, I - 1>(c, b)];
            V A[SB], B[SB];
            int m[SB];
#pragma unroll
            for (int q = 0; q < SB; ++q) {
                A[q] = x0;
                B[q] = {(T)0, (T)0};
                m[q] = 0;
            }
#pragma unroll 2
            for (int j = 1; j <= H; ++j) {
                const V a = lds[lds_index<C, I - 1>(c, b + j * NB)], d = lds[lds_index<C, I - 1>(c, b + (R - j) * NB)];
#pragma unroll
                for (int q = 0; q < SB; ++q) {
                    // s0 + q may run past H in the last group: its index stays in range (s <= H + SB - 1 < R) and
                    // its result is never stored
                    m[q] += s0 + q;
                    if (m[q] >= R) m[q] -= R;
                    const V w = cs[m[q]];  // (cos, sin)(2 pi m / R)
                    A[q].x = fma_t(w.x, a.x, A[q].x);
                    A[q].y = fma_t(w.x, a.y, A[q].y);
                    B[q].x = fma_t(w.y, d.x, B[q].x);
                    B[q].y = fma_t(w.y, d.y, B[q].y);
                }
            }
#pragma unroll
            for (int q = 0; q < SB; ++q) {
                lo[k][q] = {A[q].x + B[q].y, A[q].y - B[q].x};  // X_s
                hi[k][q] = {A[q].x - B[q].y, A[q].y + B[q].x};  // X_{R-s}
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < IPT; ++k) {
        const int id = tid + k * C::THREADS;
        if (id < ITEMS) {
            const int cb = id / GROUPS, s0 = (id - cb * GROUPS) * SB;
            const int c = cb / NB, b = cb - c * NB;
#pragma unroll
            for (int q = 0; q < SB; ++q) {
                const int s = s0 + q;
                if (s <= H) {
                    const int qq = b / P, o0 = qq * P * R + (b - qq * P);  // Stockham scatter (pass 0: P = 1)
                    lds[lds_index<C, I>(c, o0 + s * P)] = lo[k][q];
                    if (s > 0) lds[lds_index<C, I>(c, o0 + (R - s) * P)] = hi[k][q];
                }
            }
        }
    }
    __syncthreads();
}

// One sub-pass of the M-point FFT inside rader_pass.  K: pass of the split; INV: second (inverse) transform.
//   gather    K = 0 of the forward transform reads the INPUT positions of the R-point DFT through the permutation g^q
//             (times the Stockham twiddle of the enclosing pass when I > 0); every other sub-pass reads slots 1..M of the
//             DFT's OUTPUT block
//   finish    last sub-pass forward:  slot 0 <- x_0 + A[0];  A[n] <- conj(A[n] * B[n])   (B carries the 1 / M)
//             last sub-pass inverse:  X[g^-q] = x_0 + conj(d[q]) scattered through the second permutation
template <class C, int I, int K, bool INV>
MIFFT_DEV void rader_sub(cpx<typename C::T>* lds, const cpx<typename C::T>* ltw, const cpx<typename C::T>* rt, int tid) {
    using T = typename C::T;
    using V = cpx<T>;
    constexpr int R = C::R(I), M = R - 1, NB = C::NB(I), P = C::P(I), INST = C::TILE * NB;
    constexpr bool PAD = !rader_ok(R);   // convolution of length L > M in a scratch block of L elements per DFT
    constexpr int L = rader_len(R);
    constexpr RaderSplitT S = rader_split(L);
    constexpr int RK = S.r[K], NBK = L / RK;
    constexpr int PK = (K == 0 ? 1 : S.r[0]) * (K <= 1 ? 1 : S.r[1]) * (K <= 2 ? 1 : S.r[2]);  // product of the earlier radices
    constexpr int RATIO = L / (PK * RK);
    constexpr int ITEMS = INST * NBK, IPT = (ITEMS + C::THREADS - 1) / C::THREADS;
    constexpr bool LAST = K == S.np - 1;
    const V* Bt = rt;
    const V* Wm = rt + L;
    const unsigned short* perm_in = (const unsigned short*)(rt + 2 * L);
    const unsigned short* perm_out = perm_in + M;
    V* x0buf = (V*)rt + 2 * L + (4 * M + (int)sizeof(V) - 1) / (int)sizeof(V);
    V* scr = x0buf + INST;  // PAD only: [inst][L]
    // element n of the running convolution of DFT `inst` sits at blk[n * STR]: slot 1 + n of its output block in the data
    // tile (the Stockham layout is linear in n: rows stride P, column tiles P * CPITCH), or its scratch block
    constexpr int STR = PAD ? 1 : (C::COLS ? P * C::CPITCH : P);
    static_assert(PAD || C::COLS || !is_pow2_ce(C::N), "no swizzle on lengths with a prime factor above 32");
    V v[IPT][RK];
#pragma unroll
    for (int it = 0; it < IPT; ++it) {
        const int id = tid + it * C::THREADS;
        if (ITEMS % C::THREADS == 0 || id < ITEMS) {
            const int inst = id / NBK, kb = id - inst * NBK;
            const int c = inst / NB, b = inst - c * NB;
            const int q = b / P, pp = b - q * P, o0 = q * P * R + pp;
            if constexpr (K == 0 && !INV) {
#pragma unroll
                for (int t = 0; t < RK; ++t) {
                    const int qq = kb + t * NBK;
                    V u = {(T)0, (T)0};
                    if (!PAD || qq < M) {  // (padded: the sequence x[g^q] is followed by L - M zeros)
                        const int j = perm_in[qq];  // 1 .. R-1
                        u = lds[lds_index<C, I - 1>(c, b + j * NB)];
                        if constexpr (I > 0) u = cmul(u, ltw[C::TWL_OFF(I) + (j - 1) * P + pp]);
                    }
                    v[it][t] = u;
                }
                if (kb == 0) x0buf[inst] = lds[lds_index<C, I - 1>(c, b)];  // (x0buf is outside the data tile)
            } else {
                const int ppk = kb % PK;
                const V* blk = PAD ? scr + inst * L : lds + lds_index<C, I>(c, o0 + P);
#pragma unroll
                for (int t = 0; t < RK; ++t) {
                    V u = blk[(kb + t * NBK) * STR];
                    if (t > 0 && PK > 1) u = cmul(u, Wm[t * ppk * RATIO]);
                    v[it][t] = u;
                }
            }
        }
    }
    __syncthreads();  // every read of this sub-pass precedes every write (the blocks of different DFTs interleave)
#pragma unroll
    for (int it = 0; it < IPT; ++it) {
        const int id = tid + it * C::THREADS;
        if (ITEMS % C::THREADS == 0 || id < ITEMS) {
            const int inst = id / NBK, kb = id - inst * NBK;
            const int c = inst / NB, b = inst - c * NB;
            const int q = b / P, pp = b - q * P, o0 = q * P * R + pp;
            Dft<RK, T, 1>::run(v[it]);
            const int qk = kb / PK, ppk = kb - qk * PK, n0 = qk * PK * RK + ppk;  // outputs n0 + s * PK
            V* blk = PAD ? scr + inst * L : lds + lds_index<C, I>(c, o0 + P);
#pragma unroll
            for (int s2 = 0; s2 < RK; ++s2) {
                const int n = n0 + s2 * PK;
                V y = v[it][s2];
                if constexpr (LAST && !INV) {
                    if (n == 0) lds[lds_index<C, I>(c, o0)] = x0buf[inst] + y;  // X_0 = x_0 + sum of the others
                    y = cmul(y, Bt[n]);
                    y.y = -y.y;
                    blk[n * STR] = y;
                } else if constexpr (LAST && INV) {
                    y.y = -y.y;
                    if (!PAD || n < M) lds[lds_index<C, I>(c, o0 + (int)perm_out[n] * P)] = x0buf[inst] + y;
                } else {
                    blk[n * STR] = y;
                }
            }
        }
    }
    __syncthreads();
    if constexpr (!LAST) rader_sub<C, I, K + 1, INV>(lds, ltw, rt, tid);
}

// A prime radix R > 32 (C::RADER(I)): Rader's algorithm inside the LDS tile; replaces bigprime_pass.  In place in the DFT's
// output block when R - 1 splits into register butterflies, through a zero-padded convolution in a scratch block otherwise.
// Inputs at positions b + j NB of the staged / previous layout, outputs at the Stockham positions q P R + p + s P.
template <class C, int I>
MIFFT_DEV void rader_pass(cpx<typename C::T>* lds, const cpx<typename C::T>* ltw, const cpx<typename C::T>* rt, int tid) {
    rader_sub<C, I, 0, false>(lds, ltw, rt, tid);  // A = FFT_M(x[g^q]);  slot 0 <- X_0;  slots 1.. <- conj(A B)
    rader_sub<C, I, 0, true>(lds, ltw, rt, tid);   // d = FFT_M(.);  X[g^-q] = x_0 + conj(d[q])
}

// 1: the next tile's HBM loads are issued in slices between the passes of the current tile; 0: all at the top
#ifndef MIFFT_SLICED_PREFETCH
#define MIFFT_SLICED_PREFETCH 1
#endif
#ifndef MIFFT_SLICED_PREFETCH_PLANE
#define MIFFT_SLICED_PREFETCH_PLANE 1
#endif

template <int K>
struct IntC {
    static constexpr int value = K;
};

struct NoHook {
    MIFFT_DEV void operator()() const {}
    template <int K>
    MIFFT_DEV void operator()(IntC<K>) const {}
};

// TWSHIFT: extra offset of this configuration's LDS twiddle table (rectangular planes keep two tables)
// `before_stores` runs once per tile, after the last LDS read and right BEFORE the butterflies + HBM stores of the last
// pass: the prefetching kernels wait there for the next tile's inputs (loads issued a whole tile earlier: the wait is
// free).  vmcnt counts loads and stores together and the compiler's s_waitcnt insertion cannot count the exec-masked
// stores, so without this the wait for the prefetched registers -- at the top of the next iteration -- was a vmcnt(0):
// it waited for every store of the tile just finished before the next loads were even issued (29 % of the tile period
// of the 640-point column tile by in-kernel stamps).  After an explicit, compiler-visible vmcnt(0) ahead of the stores
// the registers are known to be loaded and the top-of-loop copy needs no wait at all.
// `between(IntC<K>)` runs at the seams of the tile: K = 2 I + 1 behind the barrier that follows the scatter of pass I,
// K = 2 I behind the barrier that follows the gather of pass I (1 <= I < NP - 1).  The prefetching kernels issue the
// next tile's HBM loads there in SLICES.  Issued in one burst (at the top of the tile, or anywhere else) the 20 loads
// per thread of a 640-point column tile take ~5 000 cycles to be ACCEPTED -- every wave of the one workgroup a CU holds
// sits in that issue stall at once, and nothing computes meanwhile (in-kernel stamps: the stall moves with the burst,
// 4 500 of 16 600 cycles per tile).  A few loads per seam keep the vector-memory queue short, the waves go on to their
// butterflies, and the memory system sees a steady stream instead of load / compute / store phases.
template <class C, int I, int TWSHIFT = 0, class Hook = NoHook, class Hook0 = NoHook>
MIFFT_DEV void run_pass(const TileParams& p, cpx<typename C::T>* lds, const cpx<typename C::T>* twr,
                        cpx<typename C::T> (*pre)[C::R(0)], long long base, int nv, int tid, long long obase = 0,
                        int fs_row = 0, Hook before_stores = Hook(), Hook0 between = Hook0()) {
    if constexpr (I < C::NP && C::RADER(I)) {
        rader_pass<C, I>(lds, lds + C::DATA_ELEMS + TWSHIFT, lds + C::DATA_ELEMS + C::TWL_TOTAL + C::CS_OFF(I), tid);
        run_pass<C, I + 1, TWSHIFT>(p, lds, twr, pre, base, nv, tid, obase, fs_row, before_stores, between);
    } else if constexpr (I < C::NP && C::BIGP(I)) {
        bigprime_pass<C, I>(lds, lds + C::DATA_ELEMS + TWSHIFT, lds + C::DATA_ELEMS + C::TWL_TOTAL + C::CS_OFF(I), tid);
        run_pass<C, I + 1, TWSHIFT>(p, lds, twr, pre, base, nv, tid, obase, fs_row, before_stores, between);
    } else if constexpr (I < C::NP) {
        using T = typename C::T;
        using V = cpx<T>;
        constexpr int R = C::R(I), IPT = C::IPT(I);
        constexpr bool SRC_GLOBAL = (I == 0) && C::FIRST_DIRECT;
        constexpr bool DST_GLOBAL = (I == C::NP - 1) && C::LAST_DIRECT;
        V v[IPT][R];
        if constexpr (SRC_GLOBAL) {
            if constexpr (C::PREFETCH) {
#pragma unroll
                for (int k = 0; k < IPT; ++k)
#pragma unroll
                    for (int j = 0; j < R; ++j) v[k][j] = pre[k][j];
            } else {
                load_pass0<C>(p, v, base, nv, tid);
            }
            // inverse = conj(F(conj x)) / N.  A real input is its own conjugate: its imaginary parts stay the CONSTANT +0,
            // which lets the compiler fold the imaginary half of the first butterflies away (radix 31 on real input: 176 ->
            // VGPRs, no spill; a runtime -0 / +0 kept every one of them live).
            if (p.inverse && C::CONJ_IN) {
#pragma unroll
                for (int k = 0; k < IPT; ++k)
#pragma unroll
                    for (int j = 0; j < R; ++j) v[k][j].y = -v[k][j].y;
            }
        } else {
            pass_gather_lds<C, I>(p, lds, lds + C::DATA_ELEMS + TWSHIFT, twr, v, tid);
            // in-place LDS buffer: every read of this pass completes before any later write (this
            // pass's scatter, or pass 0 of the NEXT tile when this pass stores to HBM).  WSUB: the passes 1..NP-2
            // exchange inside wave-owned sub-problems -- only the LAST gather must hold back the other waves' next
            // tile
            if constexpr (C::WSUB && I >= 1 && I < C::NP - 1)
                wave_lds_fence();
            else
                wg_barrier<C>();
            if constexpr (I < C::NP - 1) between(IntC<2 * I>{});
        }
        MIFFT_STAMP(C, 1 + 4 * I);  // gather (+ its barrier) of pass I: LDS reads / twiddles / wait for HBM loads
        if constexpr (I == C::NP - 1) before_stores();
        pass_compute_scatter<C, I>(p, lds, v, base, nv, tid, obase, fs_row);
        MIFFT_STAMP(C, 2 + 4 * I);  // butterflies + scatter issue of pass I
        if constexpr (!DST_GLOBAL) {
            if constexpr (C::WSUB && I >= 1 && I < C::NP - 1)
                wave_lds_fence();
            else
                wg_barrier<C>();
        }
        MIFFT_STAMP(C, 3 + 4 * I);  // barrier after the scatter of pass I
        if constexpr (!DST_GLOBAL && I < C::NP - 1) between(IntC<2 * I + 1>{});
        run_pass<C, I + 1, TWSHIFT>(p, lds, twr, pre, base, nv, tid, obase, fs_row, before_stores, between);
    }
}

// ---- the stages the walks below share (wgrad_walk, part_walk, pair_walk) --------------------------------------------------------
// (Hoisted out of wgrad_walk and part_walk with their instructions kept: the reference parameters of the load and the store,
//  the scaled samples as the store's arguments and the operand order of unpack_bins' twiddle products are what made the
//  compiler emit the same code for those two walks as before -- DESIGN.md 3.4w.)
// One packed element of a zero-extended row: the samples i and i + 1 of the `len` reals at xe, zeros outside [0, len) and never
// loaded there; a pair load where both lie inside (aligned to one element), real by real at the ends.  The ungated load: a
// pregate's second stream of loads stays with the two walks that have one.
template <class C, typename I>
MIFFT_DEV cpx<typename C::T> load_embedded(const typename C::IT* const& xe, const I& i, const int& len) {
    using T = typename C::T;
    cpx<T> v = {(T)0, (T)0};
    if (i >= 0 && i + 1 < len) {
        v = sload_pair<T>(xe + i);
    } else {  // (zeros beyond the ends: no load at all)
        if (i >= 0 && i < len) v.x = sload<T>(xe + i);
        if (i + 1 >= 0 && i + 1 < len) v.y = sload<T>(&xe[i + 1]);
    }
    return v;
}

// X[k] and X[N-k] of row c of the tile from the packed spectrum its last pass left in LDS, as the R2C store unpacks them
// (w: W_2N^k, TileParams::r2c_tw)
template <class C>
MIFFT_DEV void unpack_bins(const cpx<typename C::T>* lds, const cpx<typename C::T>* w, const int c, const int k,
                           cpx<typename C::T>& xa, cpx<typename C::T>& xb) {
    using T = typename C::T;
    using V = cpx<T>;
    const int m = k ? C::N - k : 0;
    const V zk = lds[lds_index<C, C::NP - 1>(c, k)], zm = lds[lds_index<C, C::NP - 1>(c, m)];
    const T ex = (T)0.5 * (zk.x + zm.x), ey = (T)0.5 * (zk.y - zm.y);
    const T ox = (T)0.5 * (zk.y + zm.y), oy = (T)-0.5 * (zk.x - zm.x);
    const V wk = w[k];
    const T tx = ox * wk.x - oy * wk.y, ty = oy * wk.x + ox * wk.y;
    xa = {ex + tx, ey + ty};
    xb = {ex - tx, ty - ey};
}

// The C2R fold of the bins a = Y[k], b = Y[N-k] of row c, as the CONV product stage folds one product: conj Z of the packed row
// goes to the slots k and N - k of the layout pass 0 gathers from (the imaginary parts of bins 0 and N dropped)
template <class C>
MIFFT_DEV void fold_bins(cpx<typename C::T>* lds, const cpx<typename C::T>* w, const int c, const int k, cpx<typename C::T> a,
                         cpx<typename C::T> b) {
    using T = typename C::T;
    const int m = k ? C::N - k : 0;
    if (k == 0) a.y = b.y = (T)0;
    const cpx<T> wk = w[k];
    const T fx = a.x + b.x, fy = a.y - b.y, dx = a.x - b.x, dy = a.y + b.y;
    const T px = dx * wk.x + dy * wk.y, py = dy * wk.x - dx * wk.y;
    lds[lds_index<C, C::NP - 1>(c, k)] = {fx - py, -(fy + px)};
    if (k != 0 && 2 * k != C::N) lds[lds_index<C, C::NP - 1>(c, m)] = {fx + py, fy - px};
}

// The store of the two finished samples of one packed element: y0 (wanted: w0) and y1 (w1) go to q[0] and q[1], as one access
// where both are wanted and q is aligned to two elements, else real by real.  The ungated store: a postgate's loads stay with
// the walk that has one.
template <class C>
MIFFT_DEV void store_window(typename C::IT* const& q, const bool& w0, const bool& w1, const typename C::T& y0,
                            const typename C::T& y1) {
    using ST = typename C::IT;
    if (w0 && w1 && ((unsigned long long)q & (2 * sizeof(ST) - 1)) == 0) {
        sstore_pair(q, y0, y1);
    } else {
        if (w0) sstore(q, y0);
        if (w1) sstore(q + 1, y1);
    }
}

// The walk of a TileCfg::WGRAD workgroup (see there): the whole kernel body behind the table set-up.
template <class C>
MIFFT_DEV void wgrad_walk(const TileParams& p, cpx<typename C::T>* lds, const cpx<typename C::T>* twr, const int tid_entry) {
    using T = typename C::T;
    using ST = typename C::IT;  // (the storage type of x and gy: TileCfg::CONV)
    using V = cpx<T>;
    constexpr int PAIRS = C::N / 2 + 1;
    constexpr int IT = (C::TILE * PAIRS + C::THREADS - 1) / C::THREADS;
    const int D = p.conv_D, P = p.wgrad_partials;
    const int d = (int)blockIdx.x / P, sl = (int)blockIdx.x - d * P;
    // slice sl of the channel's pairs: a contiguous ascending range
    const long long Q = p.n_rows, len = Q / P, rem = Q - len * P;
    long long q = sl * len + (sl < rem ? sl : rem);
    const long long q_end = q + len + (sl < rem ? 1 : 0);
    const int F = C::OLS ? p.ols_blocks : 1, S = p.ols_step, s0 = C::OLS ? p.ols_start : 0;
    const int c0 = p.conv_o, Lo = p.conv_Lo, L = p.conv_len;
    const ST* x = (const ST*)p.in;
    const ST* gy = (const ST*)p.gate_in;
    const ST* ga0 = (C::GATE & 1) ? (const ST*)p.wgrad_pregate : x;  // (the gates of the same rows; else unused)
    const ST* gb0 = (C::GATE & 2) ? (const ST*)p.gate_out : gy;
    const V* w = (const V*)p.r2c_tw;
    V acc_a[IT], acc_b[IT];
#pragma unroll
    for (int i = 0; i < IT; ++i) acc_a[i] = acc_b[i] = {(T)0, (T)0};
    V cur[1][C::R(0)];
    int tid = tid_entry;
    // X[k] and X[N-k] of the row the item owns, as the R2C store unpacks them (zeros past the last item)
    auto unpack = [&](int i, V& xa, V& xb) {
        const int f = tid + i * C::THREADS;
        xa = xb = {(T)0, (T)0};
        if (IT * C::THREADS == C::TILE * PAIRS || f < C::TILE * PAIRS) {
            const int c = f / PAIRS, k = f - c * PAIRS;
            unpack_bins<C>(lds, w, c, k, xa, xb);
        }
    };
    // TileCfg::WSPEC: the bins of the step's nv live pairs, as unpacked, to row (signal row) F + block of `out`; consecutive
    // work items hold consecutive bins k of one row, so the stores of X[k] run up whole lines and those of X[N-k] down them
    auto store_bins = [&](int nv, long long b0, int fr0) {
        V* const so = (V*)p.out;
#pragma unroll
        for (int i = 0; i < IT; ++i) {
            const int f = tid + i * C::THREADS;
            V xa, xb;
            unpack(i, xa, xb);
            if (IT * C::THREADS == C::TILE * PAIRS || f < C::TILE * PAIRS) {
                const int c = f / PAIRS, k = f - c * PAIRS;
                if (c < nv) {
                    int fr = fr0 + c, db = 0;
                    if (fr >= F) {
                        db = fr / F;
                        fr -= db * F;
                    }
                    V* const row = so + (((b0 + db) * D + d) * F + fr) * (long long)(C::N + 1);
                    row[k] = xa;
                    if (2 * k != C::N) row[C::N - k] = xb;  // (k = 0: bin N)
                }
            }
        }
    };
    for (; q < q_end; q += C::TILE) {
        const int nv = q_end - q < C::TILE ? (int)(q_end - q) : C::TILE;
        tid = tid_entry;  // (opaque once per step, as in tile_kernel: the offsets derived from it are not kept live across steps)
#ifndef MIFFT_NO_OPAQUE_TID
        if constexpr (C::OPAQUE_TID) asm volatile("" : "+v"(tid));
#endif
        // (signal of the channel, block) of the tile's first pair once, uniform; a pair further on wraps into the next signals
        const long long b0 = q / F;
        const int fr0 = (int)(q - b0 * F);
        // u-blocks: packed element m of pair c holds the samples s0 + fr S + 2 m and + 1 of its row, zeros outside [0, L)
        // (WSPEC = 2 stores the spectra of the g-blocks: no u-block is loaded)
        for (int f = tid; C::WSPEC != 2 && f < C::TILE * C::N; f += C::THREADS) {
            const int c = f / C::N, m = f - c * C::N;
            V v = {(T)0, (T)0};
            if (c < nv) {
                int fr = fr0 + c, db = 0;
                if (fr >= F) {
                    db = fr / F;
                    fr -= db * F;
                }
                const long long row = ((b0 + db) * D + d) * (long long)L;
                const ST* xe = x + row;
                const ST* ae = ga0 + row;
                const int i = s0 + fr * S + 2 * m;
                if constexpr (C::GATE & 1) {
                    if (i >= 0 && i + 1 < L) {
                        v = sload_pair<T>(xe + i);
                        const V g = sload_pair<T>(ae + i);
                        v = {g.x * v.x, g.y * v.y};
                    } else {  // (zeros beyond the ends: no load at all, of x or of its gate)
                        if (i >= 0 && i < L) {
                            v.x = sload<T>(xe + i);
                            v.x = sload<T>(ae + i) * v.x;
                        }
                        if (i + 1 >= 0 && i + 1 < L) {
                            v.y = sload<T>(&xe[i + 1]);
                            v.y = sload<T>(&ae[i + 1]) * v.y;
                        }
                    }
                } else {
                    v = load_embedded<C>(xe, i, L);
                }
            }
            lds[lds_index<C, -1>(c, m)] = v;
        }
        if constexpr (C::WSPEC != 2) {
            __syncthreads();
            run_pass<C, 0>(p, lds, twr, cur, 0, C::TILE, tid);
        }
        if constexpr (C::WSPEC == 1) {
            store_bins(nv, b0, fr0);
            __syncthreads();
            continue;
        }
        V ua[IT], ub[IT];
        if constexpr (C::WSPEC == 0) {
#pragma unroll
            for (int i = 0; i < IT; ++i) unpack(i, ua[i], ub[i]);
            __syncthreads();
        }
        // g-blocks: sample i of the block is gy[row][fr S + i - c] for c <= i < c + S and fr S + i - c < Lo, zero elsewhere
        for (int f = tid; f < C::TILE * C::N; f += C::THREADS) {
            const int c = f / C::N, m = f - c * C::N;
            V v = {(T)0, (T)0};
            if (c < nv) {
                int fr = fr0 + c, db = 0;
                if (fr >= F) {
                    db = fr / F;
                    fr -= db * F;
                }
                const int u = 2 * m - c0, t = fr * S + u;
                const bool w0 = u >= 0 && u < S && t < Lo, w1 = u + 1 >= 0 && u + 1 < S && t + 1 < Lo;
                const long long row = ((b0 + db) * D + d) * (long long)Lo;
                const ST* ge = gy + row;
                const ST* be = gb0 + row;  // (the postgate in gy's coordinates: the same (row, t))
                if (w0 && w1) {
                    v = sload_pair<T>(ge + t);
                    if constexpr (C::GATE & 2) {
                        const V g = sload_pair<T>(be + t);
                        v = {g.x * v.x, g.y * v.y};
                    }
                } else {
                    if (w0) {
                        v.x = sload<T>(ge + t);
                        if constexpr (C::GATE & 2) v.x = sload<T>(be + t) * v.x;
                    }
                    if (w1) {
                        v.y = sload<T>(&ge[t + 1]);
                        if constexpr (C::GATE & 2) v.y = sload<T>(&be[t + 1]) * v.y;
                    }
                }
            }
            lds[lds_index<C, -1>(c, m)] = v;
        }
        __syncthreads();
        run_pass<C, 0>(p, lds, twr, cur, 0, C::TILE, tid);
        if constexpr (C::WSPEC == 2) {
            store_bins(nv, b0, fr0);
            __syncthreads();
            continue;
        }
#pragma unroll
        for (int i = 0; i < IT; ++i) {
            V ga, gb;
            unpack(i, ga, gb);
            // conj(U) G
            acc_a[i].x += ua[i].x * ga.x + ua[i].y * ga.y;
            acc_a[i].y += ua[i].x * ga.y - ua[i].y * ga.x;
            acc_b[i].x += ub[i].x * gb.x + ub[i].y * gb.y;
            acc_b[i].y += ub[i].x * gb.y - ub[i].y * gb.x;
        }
        __syncthreads();
    }
    if constexpr (C::WSPEC != 0) return;  // (every bin is in memory: nothing was summed)
    // the TILE rows in ascending order, through the tile's LDS: first the bins k, then the bins N - k
    V* out =(V*)p.out + ((long long)sl * D + d) * (C::N + 1);
    const T cj = (p.conv_mode & 1) ? (T)-1 : (T)1;
    static_assert(C::TILE * PAIRS <= C::DATA_ELEMS, "WGRAD: one accumulator per (row, bin pair) fits the tile");
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
        for (int i = 0; i < IT; ++i) {
            const int f = tid + i * C::THREADS;
            if (IT * C::THREADS == C::TILE * PAIRS || f < C::TILE * PAIRS) lds[f] = half ? acc_b[i] : acc_a[i];
        }
        __syncthreads();
        for (int k = tid; k < PAIRS; k += C::THREADS) {
            V s = lds[k];
            for (int c = 1; c < C::TILE; ++c) {
                const V a = lds[c * PAIRS + k];
                s.x += a.x;
                s.y += a.y;
            }
            s.y *= cj;
            if (half == 0)
                out[k] = s;
            else if (2 * k != C::N)
                out[C::N - k] = s;  // (k = 0: bin N)
        }
        __syncthreads();
    }
}

// The walk of a TileCfg::PART workgroup (see there): the whole kernel body behind the table set-up.
template <class C>
MIFFT_DEV void part_walk(const TileParams& p, cpx<typename C::T>* lds, const cpx<typename C::T>* twr, const int tid_entry) {
    using T = typename C::T;
    using ST = typename C::IT;  // (the storage type of x, the gates and out: TileCfg::CONV)
    using V = cpx<T>;
    constexpr int PAIRS = C::N / 2 + 1, NN = 2 * C::N;
    constexpr int IT = (C::TILE * PAIRS + C::THREADS - 1) / C::THREADS;
    const int D = p.conv_D, Q = p.conv_Q, P = p.conv_parts;
    const int F = p.ols_blocks, S = p.ols_step, s0 = p.ols_start, len = p.conv_len;
    const int o = p.conv_o, Lo = p.conv_Lo;
    const bool corr = (p.conv_mode & 1) != 0;
    const T cj = corr ? (T)-1 : (T)1;
    const T s = (T)p.scale;
    const V* w = (const V*)p.r2c_tw;
    const V* hs = (const V*)p.conv_h;
    V cur[1][C::R(0)];
    for (long long t = blockIdx.x; t < p.n_tiles; t += gridDim.x) {
        // (the thread index is made opaque once per PARTITION and once more for the fold and the store: what is derived from
        //  it -- LDS and spectrum offsets, the twiddles w[k] -- is then recomputed per partition instead of staying live
        //  across the passes beside the accumulators; see tile_kernel)
        // A block's work is its live partitions, which grow with f (correlation: shrink): walked row by row, a grid whose size
        // is a multiple of F would hand one workgroup the same f every round.  One-row tiles are therefore walked block-major,
        // the dearest f of every signal first: position t is block t / signals (from the dear end) of signal t % signals.
        long long r0 = t * C::TILE;
        if constexpr (C::TILE == 1) {
            const long long ns = p.n_rows / F, rk = t / ns;
            r0 = (t - rk * ns) * F + (corr ? rk : F - 1 - rk);
        }
        const long long b0 = r0 / F;
        const int nv = p.n_rows - r0 < C::TILE ? (int)(p.n_rows - r0) : C::TILE;
        // (signal, block) of the tile's first row once, uniform; a row further on wraps into the signals that follow
        const int fr0 = (int)(r0 - b0 * F);
        const ST* x0 = (const ST*)p.in + b0 * len;
        const ST* g0 = (C::GATE & 1) ? (const ST*)p.gate_in + b0 * len : x0;  // (the gate of the same signal row; else unused)
        const unsigned d0 = (unsigned)(((long long)p.conv_row0 + b0) % (long long)D);  // (uniform; d0 + c < 2^31)
        // first sample of the block that row c of the tile loads for partition pp (|.| < 2^31: T, P Q <= 2^30, F S < T + 2N);
        // the block holds a sample of its row when it starts after -n and before T
        auto start = [&](int c, int pp) -> long long {
            int fr = fr0 + c;
            if (fr >= F) fr -= fr / F * F;
            return (long long)s0 + (long long)fr * S + (corr ? (long long)pp * Q : -(long long)pp * Q);
        };
        auto live = [&](long long st) { return st > -(long long)NN && st < (long long)len; };
        V acc_a[IT], acc_b[IT];
#pragma unroll
        for (int i = 0; i < IT; ++i) acc_a[i] = acc_b[i] = {(T)0, (T)0};
#pragma unroll 1
        for (int pp = 0; pp < P; ++pp) {
            unsigned long long alive = 0;  // (uniform: every work item walks the same rows; bit c: row c reads a sample)
            for (int c = 0; c < nv; ++c) alive |= (unsigned long long)live(start(c, pp)) << c;
            if (!alive) continue;
            int tid = tid_entry;
#ifndef MIFFT_NO_OPAQUE_TID
            asm volatile("" : "+v"(tid));  // (at every length: the accumulators leave less room than a plain tile has)
#endif
            // packed element m of row c: the samples st + 2 m and st + 2 m + 1 of its signal, zeros outside [0, T)
            for (int f = tid; f < C::TILE * C::N; f += C::THREADS) {
                const int c = f / C::N, m = f - c * C::N;
                V x = {(T)0, (T)0};
                if (c < nv) {
                    const int db = fr0 + c >= F ? (fr0 + c) / F : 0;
                    const ST* xe = x0 + (long long)db * len;
                    const ST* ge = g0 + (long long)db * len;
                    const long long i = start(c, pp) + 2 * m;
                    if constexpr (C::GATE & 1) {
                        if (i >= 0 && i + 1 < len) {
                            x = sload_pair<T>(xe + i);
                            const V g = sload_pair<T>(ge + i);
                            x = {g.x * x.x, g.y * x.y};
                        } else {  // (zeros beyond the ends: no load at all, of x or of its gate)
                            if (i >= 0 && i < len) {
                                x.x = sload<T>(xe + i);
                                x.x = sload<T>(ge + i) * x.x;
                            }
                            if (i + 1 >= 0 && i + 1 < len) {
                                x.y = sload<T>(&xe[i + 1]);
                                x.y = sload<T>(&ge[i + 1]) * x.y;
                            }
                        }
                    } else {
                        x = load_embedded<C>(xe, i, len);
                    }
                }
                lds[lds_index<C, -1>(c, m)] = x;
            }
            __syncthreads();
            run_pass<C, 0>(p, lds, twr, cur, 0, C::TILE, tid);
#pragma unroll
            for (int i = 0; i < IT; ++i) {
                const int f = tid + i * C::THREADS;
                if ((IT * C::THREADS == C::TILE * PAIRS || f < C::TILE * PAIRS) && f < nv * PAIRS) {
                    const int c = C::TILE == 1 ? 0 : f / PAIRS, k = f - c * PAIRS, m = k ? C::N - k : 0;
                    if ((alive >> c) & 1) {
                        const unsigned dc = fr0 + c >= F ? (unsigned)(fr0 + c) / (unsigned)F : 0u;
                        const V* hr = hs + ((long long)((d0 + dc) % (unsigned)D) * P + pp) * (C::N + 1);
                        const V ga = hr[k], gb = hr[C::N - k];  // (k = 0: bin N, the last of the row)
                        const V zk = lds[lds_index<C, C::NP - 1>(c, k)], zm = lds[lds_index<C, C::NP - 1>(c, m)];
                        // X[k] and X[N-k], as the R2C store unpacks them
                        const T ex = (T)0.5 * (zk.x + zm.x), ey = (T)0.5 * (zk.y - zm.y);
                        const T ox = (T)0.5 * (zk.y + zm.y), oy = (T)-0.5 * (zk.x - zm.x);
                        const V wk = w[k];
                        const T tx = wk.x * ox - wk.y * oy, ty = wk.x * oy + wk.y * ox;
                        const V xa = {ex + tx, ey + ty}, xb = {ex - tx, ty - ey};
                        // times H (conjugated: correlation)
                        const V pa = cmul(xa, V{ga.x, cj * ga.y}), pb = cmul(xb, V{gb.x, cj * gb.y});
                        acc_a[i].x += pa.x;
                        acc_a[i].y += pa.y;
                        acc_b[i].x += pb.x;
                        acc_b[i].y += pb.y;
                    }
                }
            }
            __syncthreads();
        }
        int tid = tid_entry;
#ifndef MIFFT_NO_OPAQUE_TID
        asm volatile("" : "+v"(tid));
#endif
        // the C2R fold of the sums, as the CONV product stage folds one product (rows from nv on: zeros)
#pragma unroll
        for (int i = 0; i < IT; ++i) {
            const int f = tid + i * C::THREADS;
            if (IT * C::THREADS == C::TILE * PAIRS || f < C::TILE * PAIRS) {
                const int c = C::TILE == 1 ? 0 : f / PAIRS, k = f - c * PAIRS;
                fold_bins<C>(lds, w, c, k, acc_a[i], acc_b[i]);
            }
        }
        __syncthreads();
        run_pass<C, 0>(p, lds, twr, cur, 0, C::TILE, tid);
        // the OLS store: sample i of block fr goes to out[b Lo + fr S + i - c] for c <= i < c + S and fr S + i - c < Lo only
        ST* out0 = (ST*)p.out + b0 * Lo;
        const ST* q0 = (C::GATE & 2) ? (const ST*)p.gate_out + b0 * Lo : out0;  // (else unused)
        for (int f = tid; f < nv * C::N; f += C::THREADS) {
            const int c = f / C::N, j = f - c * C::N, u = 2 * j - o;
            if (u + 1 < 0 || u >= S) continue;
            int fr = fr0 + c, db = 0;
            if (fr >= F) {
                db = fr / F;
                fr -= db * F;
            }
            const int tt = fr * S + u;  // (< Lo + 2N: 32 bits hold it)
            const bool w0 = u >= 0 && tt < Lo, w1 = u + 1 < S && tt + 1 < Lo;
            if (!w0 && !w1) continue;
            const V v = lds[lds_index<C, C::NP - 1>(c, j)];
            T y0 = v.x * s, y1 = -(v.y * s);
            ST* q = out0 + (long long)db * Lo + tt;
            if constexpr (C::GATE & 2) {
                const ST* bq = q0 + (long long)db * Lo + tt;
                if (w0 && w1 && ((unsigned long long)q & (2 * sizeof(ST) - 1)) == 0) {
                    const V g = sload_pair<T>(bq);
                    y0 = g.x * y0, y1 = g.y * y1;
                    sstore_pair(q, y0, y1);
                } else {
                    if (w0) {
                        y0 = sload<T>(bq) * y0;
                        sstore(q, y0);
                    }
                    if (w1) {
                        y1 = sload<T>(bq + 1) * y1;
                        sstore(q + 1, y1);
                    }
                }
            } else {
                store_window<C>(q, w0, w1, y0, y1);
            }
        }
        __syncthreads();
    }
}

// The walk of a TileCfg::PAIR workgroup (see there): the whole kernel body behind the table set-up.
template <class C>
MIFFT_DEV void pair_walk(const TileParams& p, cpx<typename C::T>* lds, const cpx<typename C::T>* twr, const int tid_entry) {
    using T = typename C::T;
    using ST = typename C::IT;
    using V = cpx<T>;
    constexpr int PAIRS = C::N / 2 + 1;
    constexpr int IT = (C::TILE * PAIRS + C::THREADS - 1) / C::THREADS;
    const int L = p.conv_len, K = p.pair_K, ea = p.pair_ea, eb = p.pair_eb, o = p.conv_o, Lo = p.conv_Lo;
    const T cj = (p.conv_mode & 1) ? (T)-1 : (T)1;
    const T s = (T)p.scale;
    const V* w = (const V*)p.r2c_tw;
    V cur[1][C::R(0)];
    for (long long t = blockIdx.x; t < p.n_tiles; t += gridDim.x) {
        const long long r0 = t * C::TILE;
        const int nv = p.n_rows - r0 < C::TILE ? (int)(p.n_rows - r0) : C::TILE;
        const ST* x0 = (const ST*)p.in + r0 * L;
        const ST* v0 = (const ST*)p.gate_in + r0 * K;
        // (the thread index is made opaque once per stage, as part_walk does around its accumulators: what is derived from it --
        //  LDS offsets, the twiddles w[k] -- is recomputed per stage instead of staying live beside the held bins of x)
        int tid = tid_entry;
#ifndef MIFFT_NO_OPAQUE_TID
        asm volatile("" : "+v"(tid));
#endif
        // the x-rows: packed element m of row c holds the samples 2 m - ea and 2 m + 1 - ea of its row
        for (int f = tid; f < C::TILE * C::N; f += C::THREADS) {
            const int c = f / C::N, m = f - c * C::N;
            V e = {(T)0, (T)0};
            if (c < nv) e = load_embedded<C>(x0 + c * L, 2 * m - ea, L);
            lds[lds_index<C, -1>(c, m)] = e;
        }
        __syncthreads();
        run_pass<C, 0>(p, lds, twr, cur, 0, C::TILE, tid);
        V xa[IT], xb[IT];
#pragma unroll
        for (int i = 0; i < IT; ++i) {
            const int f = tid + i * C::THREADS;
            xa[i] = xb[i] = {(T)0, (T)0};
            if (IT * C::THREADS == C::TILE * PAIRS || f < C::TILE * PAIRS) {
                const int c = C::TILE == 1 ? 0 : f / PAIRS, k = f - c * PAIRS;
                unpack_bins<C>(lds, w, c, k, xa[i], xb[i]);
            }
        }
        __syncthreads();
        tid = tid_entry;
#ifndef MIFFT_NO_OPAQUE_TID
        asm volatile("" : "+v"(tid));
#endif
        // the v-rows, the same way, into the same LDS
        for (int f = tid; f < C::TILE * C::N; f += C::THREADS) {
            const int c = f / C::N, m = f - c * C::N;
            V e = {(T)0, (T)0};
            if (c < nv) e = load_embedded<C>(v0 + c * K, 2 * m - eb, K);
            lds[lds_index<C, -1>(c, m)] = e;
        }
        __syncthreads();
        run_pass<C, 0>(p, lds, twr, cur, 0, C::TILE, tid);
        tid = tid_entry;
#ifndef MIFFT_NO_OPAQUE_TID
        asm volatile("" : "+v"(tid));
#endif
        // X G (correlation: X conj G) of both bins of the pair, folded into the two slots the item just read: it is their only reader
#pragma unroll
        for (int i = 0; i < IT; ++i) {
            const int f = tid + i * C::THREADS;
            if (IT * C::THREADS == C::TILE * PAIRS || f < C::TILE * PAIRS) {
                const int c = C::TILE == 1 ? 0 : f / PAIRS, k = f - c * PAIRS;
                V ga, gb;
                unpack_bins<C>(lds, w, c, k, ga, gb);
                fold_bins<C>(lds, w, c, k, cmul(xa[i], V{ga.x, cj * ga.y}), cmul(xb[i], V{gb.x, cj * gb.y}));
            }
        }
        __syncthreads();
        run_pass<C, 0>(p, lds, twr, cur, 0, C::TILE, tid);
        // the windowed store: sample u = 2 j - o (and u + 1) of row c goes to out[(r0 + c) Lo + u] for 0 <= u < Lo only
        ST* out0 = (ST*)p.out + r0 * Lo;
        for (int f = tid; f < nv * C::N; f += C::THREADS) {
            const int c = f / C::N, j = f - c * C::N, u = 2 * j - o;
            const bool w0 = u >= 0 && u < Lo, w1 = u + 1 >= 0 && u + 1 < Lo;
            if (!w0 && !w1) continue;
            const V e = lds[lds_index<C, C::NP - 1>(c, j)];
            ST* q = out0 + (long long)c * Lo + u;
            store_window<C>(q, w0, w1, e.x * s, -(e.y * s));
        }
        __syncthreads();
    }
}

template <class C>
__global__ __launch_bounds__(C::THREADS, C::MINW) void tile_kernel(const TileParams p) {
    using T = typename C::T;
    using V = cpx<T>;
#ifdef MIFFT_STATIC_LDS  // runtime-compiled instances (kernels_jit.cpp): no per-function dynamic-LDS opt-in needed
    __shared__ __attribute__((aligned(16))) unsigned char smem[C::LDS_BYTES];
#else
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
#endif
    V* lds = (V*)smem;
    const int tid0 = threadIdx.x;
    V twr[(C::TWMODE == TW_REG && C::TW_TOTAL > 0) ? C::TW_TOTAL : 1];
    if constexpr (C::TWMODE == TW_REG) preload_tw<C, 1>(twr, (const V*)p.tw, tid0, p.inverse);
    if constexpr (C::TWMODE == TW_LDS) {
        fill_lds_tw<C, 1>(lds + C::DATA_ELEMS, (const V*)p.tw, tid0, p.inverse);
        // cooperative passes: (cos, sin)(2 pi m / R) from W_N^(m N/R) = cos - i sin; Rader passes: the plan's tables
        // (p.tlo: spectrum of the kernel and W_M per Rader pass, complex; p.thi: the two permutations per Rader pass, uint16)
        if constexpr (C::BIGP0 && !C::RADER(0)) {
            for (int m = tid0; m < C::R(0); m += C::THREADS) {
                V w = ((const V*)p.tw)[m * C::NB(0)];
                if (p.inverse) w.y = -w.y;
                lds[C::DATA_ELEMS + C::TWL_TOTAL + m] = {w.x, -w.y};
            }
        }
        if constexpr (C::BIGP1 && !C::RADER(1)) {
            for (int m = tid0; m < C::R(1); m += C::THREADS) {
                V w = ((const V*)p.tw)[m * C::NB(1)];
                if (p.inverse) w.y = -w.y;
                lds[C::DATA_ELEMS + C::TWL_TOTAL + C::CS_OFF(1) + m] = {w.x, -w.y};
            }
        }
        if constexpr (C::RADER(0) || C::RADER(1)) {
            // per Rader pass: complex [B (L) | W_L (L)] from p.tlo, uint16 [g^q (M) | g^-q (M)] from p.thi.  Everything here
            // is a compile-time constant (a runtime call of rader_len would factorise thousands of integers per thread)
            constexpr int L0 = C::RADER(0) ? rader_len(C::R(0)) : 0, M0 = C::RADER(0) ? C::R(0) - 1 : 0;
            constexpr int L1 = C::RADER(1) ? rader_len(C::R(1)) : 0, M1 = C::RADER(1) ? C::R(1) - 1 : 0;
            if constexpr (C::RADER(0)) {
                V* dst = lds + C::DATA_ELEMS + C::TWL_TOTAL + C::CS_OFF(0);
                for (int m = tid0; m < 2 * L0; m += C::THREADS) dst[m] = ((const V*)p.tlo)[m];
                unsigned short* pd = (unsigned short*)(dst + 2 * L0);
                for (int m = tid0; m < 2 * M0; m += C::THREADS) pd[m] = ((const unsigned short*)p.thi)[m];
            }
            if constexpr (C::RADER(1)) {
                V* dst = lds + C::DATA_ELEMS + C::TWL_TOTAL + C::CS_OFF(1);
                for (int m = tid0; m < 2 * L1; m += C::THREADS) dst[m] = ((const V*)p.tlo)[2 * L0 + m];
                unsigned short* pd = (unsigned short*)(dst + 2 * L1);
                for (int m = tid0; m < 2 * M1; m += C::THREADS) pd[m] = ((const unsigned short*)p.thi)[2 * M0 + m];
            }
        }
        __syncthreads();
    }

    MIFFT_STAMP(C, -1);
    if constexpr (C::WGRAD) {  // (the filter gradient walks pairs of blocks, not tiles of rows: its own loop)
        wgrad_walk<C>(p, lds, twr, tid0);
        return;
    }
    if constexpr (C::PART) {  // (the partitioned convolution transforms several blocks per stored one: its own loop)
        part_walk<C>(p, lds, twr, tid0);
        return;
    }
    if constexpr (C::PAIR) {  // (two signals per row: two loads and transforms per stored row: its own loop)
        pair_walk<C>(p, lds, twr, tid0);
        return;
    }
    V pre[C::PREFETCH ? C::IPT(0) : 1][C::R(0)];
    // this workgroup's tiles: t, t + t_step, ... < t_end
    long long t = blockIdx.x, t_end = p.n_tiles, t_step = gridDim.x;
    long long run_begin = 0;
    if constexpr (C::HERM_RUNS) {  // one contiguous run of tiles per workgroup (lengths differ by one at most), walked in
                                   // descending column order (HERM stores)
        const long long len = p.n_tiles / gridDim.x, rem = p.n_tiles - len * gridDim.x, w = blockIdx.x;
        run_begin = t = w * len + (w < rem ? w : rem);
        t_end = t + len + (w < rem ? 1 : 0);
        t_step = 1;
    }
    if constexpr (C::ISTFT) {  // the same runs in ASCENDING order, after the warm-up tiles of a run that starts inside an entry:
                               // the W tiles before it, W = min(g, ceil((K - 1) / TILE)), K = ceil(2 N / hop) frames per sample
        const long long len = p.n_tiles / gridDim.x, rem = p.n_tiles - len * gridDim.x, w = blockIdx.x;
        run_begin = w * len + (w < rem ? w : rem);
        t_end = run_begin + len + (w < rem ? 1 : 0);
        t_step = 1;
        const long long g = run_begin % p.tiles_per_outer;
        const long long K = (2 * C::N + p.stft_hop - 1) / p.stft_hop, W = (K - 1 + C::TILE - 1) / C::TILE;
        t = run_begin - (W < g ? W : g);
    }
    if constexpr (C::IMDCT) {  // the ISTFT's runs; a run that starts inside an entry is preceded by ONE warm-up frame (position
                               // run_begin - 1 of the walk), whose v[0 .. N) is the carry the first tile of the run needs
        const long long len = p.n_tiles / gridDim.x, rem = p.n_tiles - len * gridDim.x, w = blockIdx.x;
        run_begin = w * len + (w < rem ? w : rem);
        t_end = run_begin + len + (w < rem ? 1 : 0);
        t_step = 1;
        t = run_begin - (run_begin % p.tiles_per_outer != 0 && run_begin < t_end ? 1 : 0);
    }
    const long long t_first = t;
    // (runs: position t of the order is tile n_tiles - 1 - t, whatever p.reverse says; ISTFT: tile t)
    auto tile_at = [&](long long pos) { return (C::ISTFT || C::IMDCT) ? pos : C::HERM_RUNS ? p.n_tiles - 1 - pos : tile_id(p, pos); };
    if constexpr (C::XCD_CHUNK) {
        if (gridDim.x >= 8) {  // (smaller grids: some XCD would own tiles but no workgroup)
            const long long x = blockIdx.x & 7, slot = blockIdx.x >> 3;
            t_step = ((long long)gridDim.x - x + 7) >> 3;  // workgroups on this XCD
            t = x * p.n_tiles / 8 + slot;
            t_end = (x + 1) * p.n_tiles / 8;
        }
    }
    static_assert(!(C::PREFETCH && C::BIGP0), "prefetching kernels read pass 0 straight from HBM");
    if constexpr (C::PREFETCH) {
        if (t < t_end) {
            long long base;
            int nv;
            if constexpr (C::HERM) {
                int col0, in_row;
                tile_geom_herm<C>(p, tile_at(t), base, nv, col0, in_row);
            } else {
                tile_geom<C>(p, tile_at(t), base, nv);
            }
            load_pass0<C>(p, pre, base, nv, tid0);
        }
    }
    const int tid_entry = tid0;
    for (; t < t_end; t += t_step) {
        // The thread index is made opaque once per tile: every LDS / twiddle / HBM offset derived from it is then
        // recomputed inside the iteration (a few dozen VALU operations) instead of being hoisted out of the
        // persistent loop, where dozens of loop-invariant address registers stay live across the whole tile and
        // push the kernel over its VGPR budget.
        int tid = tid_entry;
#ifndef MIFFT_NO_OPAQUE_TID
        if constexpr (C::OPAQUE_TID) asm volatile("" : "+v"(tid));
#endif
        long long base;
        int nv;
        const long long tt = tile_at(t);
        long long obase = 0;
        int fs_row = 0;
        if constexpr (C::FS1) {
            tile_geom_fs1<C>(p, tt, base, obase, nv, fs_row);
        } else if constexpr (C::HERM) {  // image base and first column of the tile, for the mirrored stores
            int in_row;
            tile_geom_herm<C>(p, tt, base, nv, fs_row, in_row);
            obase = base - fs_row;
            // tile tt hands its first column to tile tt - 1 when that is the next of this run, covers the columns right below
            // it, and the column has a mirror image to be stored at all; the same test one tile up says whether tile tt + 1
            // did so (not across the start of a row of the last dimension: that column's mirror image is the FIRST element of
            // a row, next to nothing the neighbouring tile stores)
            if constexpr (C::HERM_RUNS) {
                const int nxt = fs_row + C::TILE;
                const bool out = t + 1 < t_end && fs_row % p.herm_d2 != 0 && herm_twice(p, fs_row);
                const bool in = t > run_begin && in_row + 1 < p.herm_tpr && nxt % p.herm_d2 != 0 && herm_twice(p, nxt);
                fs_row |= (in ? 1 << 30 : 0) | (out ? (int)(1u << 31) : 0);
            }
        } else if constexpr (C::ISTFT) {  // tile g of entry b: frames f0 = g TILE .. of that entry, never beyond it
            const long long b = tt / p.tiles_per_outer;
            const int f0 = (int)(tt - b * p.tiles_per_outer) * C::TILE;
            nv = p.stft_frames - f0 < C::TILE ? p.stft_frames - f0 : C::TILE;
            base = (b * p.stft_frames + f0) * C::N;
            obase = b;
            fs_row = f0;
        } else if constexpr (C::IMDCT) {  // as above; the warm-up position is the one frame before tile run_begin
            const long long ta = t < run_begin ? run_begin : tt, b = ta / p.tiles_per_outer;
            int f0 = (int)(ta - b * p.tiles_per_outer) * C::TILE;
            nv = p.stft_frames - f0 < C::TILE ? p.stft_frames - f0 : C::TILE;
            if (t < run_begin) {
                f0 -= 1;
                nv = 1;
            }
            base = (b * p.stft_frames + f0) * C::N;
            obase = b;
            fs_row = f0;
        } else {
            tile_geom<C>(p, tt, base, nv);
        }
        V cur[C::PREFETCH ? C::IPT(0) : 1][C::R(0)];
        // seams between passes where a slice of the next tile's loads can go: 2 NP - 3 of them, plus the top
        // (column tiles only: row tiles measured 4-8 % SLOWER sliced -- rows480 0.096 -> 0.104 ms, tools/tune GROUP 5 --
        //  while 640- and 1024-point column tiles gain 4-6 %)
        constexpr int SLICES = (C::PREFETCH && C::COLS && MIFFT_SLICED_PREFETCH && C::NP > 1) ? 2 * C::NP - 2 : 1;
        const long long tn = t + t_step;
        long long nbase = 0;
        int nnv = 0;
        if constexpr (C::PREFETCH) {
#pragma unroll
            for (int k = 0; k < C::IPT(0); ++k)
#pragma unroll
                for (int j = 0; j < C::R(0); ++j) cur[k][j] = pre[k][j];
            if (tn < t_end) {
                if constexpr (C::HERM) {
                    int col0, in_row;
                    tile_geom_herm<C>(p, tile_at(tn), nbase, nnv, col0, in_row);
                } else {
                    tile_geom<C>(p, tile_at(tn), nbase, nnv);
                }
            }
            if constexpr (SLICES == 1) {
                if (tn < t_end) load_pass0<C>(p, pre, nbase, nnv, tid);  // all of the next tile's HBM reads at once
            } else {
                if (tn < t_end) load_pass0<C, 0, SLICES>(p, pre, nbase, nnv, tid);
            }
        }
        // the other slices of the next tile's loads, one per seam between the passes (see run_pass)
        auto slice = [&](auto kc) {
            constexpr int K = decltype(kc)::value;
            if constexpr (C::PREFETCH && SLICES > 1 && K >= 1 && K < SLICES) {
                if (tn < t_end) load_pass0<C, K, SLICES>(p, pre, nbase, nnv, tid);
            }
        };
        // Run by the last pass right before its stores (see run_pass): the next tile's inputs were issued during this
        // tile, so waiting for them HERE costs little -- and it keeps the compiler's wait for them (at the copy above,
        // next iteration) from landing behind this tile's stores.
        auto drain = [&]() {
            if constexpr (C::PREFETCH) vm_drain();
        };
        if constexpr (!C::FIRST_DIRECT && C::COLS) {
            // column tile staged in LDS (a big-prime pass 0 or a paired-column DCT needs this): runs of TILE adjacent columns
            static_assert(C::BIGP0 || C::DCT != 0, "column tiles load directly unless pass 0 works in LDS");
            // DCT = 3: one item per pair of rows (k, N - k), k = 0 .. N / 2, and column; else one per element
            constexpr int LROWS = (C::DCT == 3) ? C::N / 2 + 1 : C::N;
            for (int f = tid; f < LROWS * C::TILE; f += C::THREADS) {
                const int n = f / C::TILE, c = f - n * C::TILE;
                const int cc = c < nv ? c : nv - 1;  // ragged last tile: re-read a valid column, never stored
                if constexpr (C::DCT == 3) {
                    // U[k] and U[N-k] (U[N] := 0), both runs over the lanes: Z[k] = conj(W^k) (s_k U[k] - i s U[N-k]) and
                    // Z[N-k] = i W^k (s U[N-k] - i s_k U[k]), W = W_4n^k; written conjugated (the passes run conj(F(conj Z)))
                    const V* gin = (const V*)p.in;
                    // (DST: bin j of the cosine transform lies in row N - 1 - j)
                    const V a = gload<(C::NT & 1) != 0>(gin + gaddr<C>(p, base, cc, C::DST ? C::N - 1 - n : n));
                    const V b = n ? gload<(C::NT & 1) != 0>(gin + gaddr<C>(p, base, cc, C::DST ? n - 1 : C::N - n)) : V{(T)0, (T)0};
                    const V w = ((const V*)p.dct_tw)[n];
                    const T s1 = (T)p.dct_s1, sk = n == 0 ? (T)p.dct_s0 : s1;
                    const T ar = sk * a.x, ai = sk * a.y, br = s1 * b.x, bi = s1 * b.y;
                    const T qx = ar + bi, qy = ai - br, rx = br + ai, ry = bi - ar;
                    lds[lds_index<C, -1>(c, n)] = {w.x * qx + w.y * qy, w.y * qx - w.x * qy};
                    if (n != 0 && 2 * n != C::N) lds[lds_index<C, -1>(c, C::N - n)] = {-(w.x * ry + w.y * rx), w.y * ry - w.x * rx};
                    continue;
                }
                V x;
                if constexpr (!same_t<typename C::IT, T>::value)
                    x = load_foreign<C>(p.in, gaddr<C>(p, base, cc, n));
                else if constexpr (C::IN_REAL)
                    x = {gload_real<false>((const T*)p.in + gaddr<C>(p, base, cc, n)), (T)0};
                else
                    x = gload<false>((const V*)p.in + gaddr<C>(p, base, cc, n));
                if (p.inverse && C::CONJ_IN) x.y = -x.y;
                if constexpr (C::DST) {  // (-1)^row on both columns of the pair
                    if (n & 1) x = {-x.x, -x.y};
                }
                lds[lds_index<C, -1>(c, C::DCT == 2 ? dct_elem_of<C>(n) : n)] = x;
            }
            __syncthreads();
        } else if constexpr (C::C2R) {
            // One thread per pair (k, N - k), k = 0 .. N / 2: X[k] and X[N - k] of the pitch-h row (two contiguous runs over the
            // lanes), folded into Z[k] and Z[N - k].  A fixed number of pairs per thread, in groups of G whose loads are all
            // issued before the first fold (G bounds the registers they hold); the pair index advances by a constant step (no
            // division per element).
            const V* gin = (const V*)p.in;
            const V* w = (const V*)p.r2c_tw;
            constexpr int PAIRS = C::N / 2 + 1, DC = C::THREADS / PAIRS, DK = C::THREADS - DC * PAIRS;
            constexpr int IT = (C::TILE * PAIRS + C::THREADS - 1) / C::THREADS, G = IT < 4 ? IT : 4;
            const long long row0 = base / C::N;
            const T s = p.inverse ? (T)-1 : (T)1;
            int c = tid / PAIRS, k = tid - c * PAIRS;
#pragma unroll 1
            for (int i0 = 0; i0 < IT; i0 += G) {
                int cs[G], ks[G];
                V xk[G], xm[G];
                T mk[C::ADJ >= 2 ? G : 1], mm[C::ADJ >= 2 ? G : 1];  // (ADJ >= 2: the real factors of the two bins)
#pragma unroll
                for (int j = 0; j < G; ++j) {
                    cs[j] = (IT % G == 0 || i0 + j < IT) ? c : nv;  // (past the last pair: nothing to do)
                    ks[j] = k;
                    if (cs[j] < nv) {
                        if constexpr (C::DCT == 3) {
                            // four runs of reals over the lanes: X[k] and X[N + k] ascending, X[n - k] and X[N - k] descending
                            // (k = 0: X[n] := 0, and X[N] twice)
                            // (DST: X[j] lies at n - 1 - j -- descending, ascending, ascending, descending; k = 0: X[N] twice)
                            const T* row = (const T*)p.in + (row0 + c) * (2 * C::N);
                            constexpr int NN = 2 * C::N;
                            xk[j].x = gload_real<(C::NT & 1) != 0>(row + (C::DST ? NN - 1 - k : k));
                            xk[j].y = k ? gload_real<(C::NT & 1) != 0>(row + (C::DST ? k - 1 : NN - k)) : (T)0;
                            xm[j].x = gload_real<(C::NT & 1) != 0>(row + (C::DST ? C::N - 1 + k : C::N - k));
                            xm[j].y = gload_real<(C::NT & 1) != 0>(row + (C::DST ? C::N - 1 - k : C::N + k));
                        } else {
                            const V* row = gin + (row0 + c) * p.half_pitch;
                            xk[j] = gload<(C::NT & 1) != 0>(row + k);
                            xm[j] = gload<(C::NT & 1) != 0>(row + (C::N - k));  // (k = 0: X[N], the last bin of the row)
                            if constexpr (C::ADJ >= 2) {
                                const T* mrow = (const T*)p.adj_mult + (row0 + c) * p.half_pitch;
                                mk[j] = gload_real<(C::NT & 1) != 0>(mrow + k);
                                mm[j] = gload_real<(C::NT & 1) != 0>(mrow + (C::N - k));
                            }
                        }
                    }
                    c += DC;
                    k += DK;
                    if (k >= PAIRS) {
                        k -= PAIRS;
                        ++c;
                    }
                }
#pragma unroll
                for (int j = 0; j < G; ++j) {
                    if (cs[j] < nv) {
                        const int kk = ks[j];
                        V a = xk[j], b = xm[j];
                        if constexpr (C::DCT == 3) {  // V[k] = conj(W_4n^k) (X[k] - i X[n-k]) / 2, V[N-k] likewise
                            const V* w4 = (const V*)p.dct_tw;
                            const V wa = w4[kk], wb = w4[C::N - kk];
                            const T s1 = (T)p.dct_s1, s0 = kk == 0 ? (T)p.dct_s0 : s1;
                            const T ar = s0 * a.x, ai = -s1 * a.y, br = s1 * b.x, bi = -s1 * b.y;
                            a = {wa.x * ar + wa.y * ai, wa.x * ai - wa.y * ar};
                            b = {wb.x * br + wb.y * bi, wb.x * bi - wb.y * br};
                        }
                        if constexpr (C::ADJ >= 2) {  // g[k] = m[k] X[k] (2; the factor 2 is the table's) or m[k] X[k] / |X[k]| (3)
                            T sa = mk[j], sb = mm[j];
                            if constexpr (C::ADJ == 3) {
                                const T ra = sqrt_t(fma_t(a.x, a.x, a.y * a.y)), rb = sqrt_t(fma_t(b.x, b.x, b.y * b.y));
                                sa = ra == (T)0 ? (T)0 : sa / ra;
                                sb = rb == (T)0 ? (T)0 : sb / rb;
                            }
                            a = {a.x * sa, a.y * sa};
                            b = {b.x * sb, b.y * sb};
                            // (the products stay products: rounded once, as if they had been read from memory, whatever the
                            //  contraction mode -- mode 2 equals mode 1 on the tensor 2 m X bit for bit; nothing is emitted)
#if defined(__HIP_DEVICE_COMPILE__)
                            asm volatile("" : "+v"(a.x), "+v"(a.y), "+v"(b.x), "+v"(b.y));
#endif
                        }
                        if (kk == 0) a.y = b.y = (T)0;
                        if constexpr (C::ADJ != 0) {  // bins 0 and N enter the real sum once, every other bin with its mirror image
                            if (kk == 0) {
                                a.x += a.x;
                                b.x += b.x;
                            }
                        }
                        const V wk = w[kk];
                        const T ex = a.x + b.x, ey = a.y - b.y, dx = a.x - b.x, dy = a.y + b.y;
                        const T ox = dx * wk.x + dy * wk.y, oy = dy * wk.x - dx * wk.y;  // O = D * conj(W^k)
                        // Z[k] = E + i O, Z[N - k] = conj(E) + i conj(O); stored conjugated for the inverse (conj(F(conj Z)))
                        lds[lds_index<C, -1>(cs[j], kk)] = {ex - oy, s * (ey + ox)};
                        if (kk != 0 && 2 * kk != C::N) lds[lds_index<C, -1>(cs[j], C::N - kk)] = {ex + oy, s * (ox - ey)};
                    }
                }
            }
            __syncthreads();
        } else if constexpr (C::ILV > 0) {
            ilv_load<C>(p, lds, base, nv * C::N, tid);
            __syncthreads();
        } else if constexpr (C::DCT == 2 && !C::COLS) {
            // the tile's nv * 2 N reals as one flat coalesced run; x[2j] goes to real slot j of its row, x[2j+1] to slot
            // n - 1 - j (pairs: two runs of 4-byte LDS stores, one ascending and one descending)
            constexpr bool NTL = (C::NT & 1) != 0;
            if constexpr (C::DCT_QUADS) {  // quad e of a row: z_e and z_(N-1-e)
                constexpr int H = C::N / 2;
                for (int f = tid; f < nv * H; f += C::THREADS) {
                    const int c = f / H, e = f - c * H;
                    T x[4];
                    if constexpr (!same_t<typename C::IT, T>::value) {
                        const V lo = load_foreign<C>(p.in, base + 2 * f), hi = load_foreign<C>(p.in, base + 2 * f + 1);
                        x[0] = lo.x, x[1] = lo.y, x[2] = hi.x, x[3] = hi.y;
                    } else {
                        gload4<NTL>((const T*)p.in + 2 * base + 4 * (long long)f, x);
                    }
                    lds[lds_index<C, -1>(c, e)] = {x[0], x[2]};
                    if constexpr (C::DST)  // the odd samples, negated: the whole element
                        lds[lds_index<C, -1>(c, C::N - 1 - e)] = {-x[3], -x[1]};
                    else
                        lds[lds_index<C, -1>(c, C::N - 1 - e)] = {x[3], x[1]};
                }
            } else {
                T* ldr = (T*)lds;
                for (int f = tid; f < nv * C::N; f += C::THREADS) {
                    const int c = f / C::N, j = f - c * C::N, q = 2 * C::N - 1 - j;
                    V x;
                    if constexpr (!same_t<typename C::IT, T>::value)
                        x = load_foreign<C>(p.in, base + f);
                    else
                        x = gload<NTL>((const V*)p.in + base + f);
                    ldr[2 * lds_index<C, -1>(c, j >> 1) + (j & 1)] = x.x;
                    ldr[2 * lds_index<C, -1>(c, q >> 1) + (q & 1)] = C::DST ? -x.y : x.y;  // (DST: the odd sample, negated)
                }
            }
            __syncthreads();
        } else if constexpr (C::DCT == 4) {
            // item (c, m), m < ceil(N / 2): a = (x[2m], x[2m+1]) and b = (x[n-2-2m], x[n-1-2m]) of row c -- of the row as it
            // lies in memory, or of the folded frame u (MDCT) -- become p_m z_m and p_(N-1-m) z_(N-1-m) in LDS
            constexpr int H2 = (C::N + 1) / 2, NN = 2 * C::N;
            const V* pw = (const V*)p.dct_tw;
            const long long row0 = base / C::N;
            // MDCT: (b, frame) of the tile's first row once, uniform; a row further on wraps into the entries that follow
            long long b0 = 0;
            int fr0 = 0;
            if constexpr (C::MDCT) {
                b0 = row0 / p.stft_frames;
                fr0 = (int)(row0 - b0 * p.stft_frames);
            }
            for (int f = tid; f < nv * H2; f += C::THREADS) {
                const int c = f / H2, m = f - c * H2;
                V a, b;
                if constexpr (C::MDCT) {
                    constexpr int h = C::N;  // (a quarter of the frame: M = 2 h coefficients, 4 h samples)
                    const int F = p.stft_frames, len = p.stft_len;
                    int fr = fr0 + c, db = 0;
                    if (fr >= F) {
                        db = fr / F;
                        fr -= db * F;
                    }
                    const T* xe = (const T*)p.in + (b0 + db) * (long long)len;
                    const long long s0 = ((long long)fr - 1) * NN;  // the frame's first sample, in [-M, T)
                    const T* win = (const T*)p.stft_win;
                    if (s0 >= 0 && s0 + 2 * NN <= len && 2 * m + 1 < h) {
                        const T* xs = xe + s0;
                        const V d1 = gload_pair(xs + 3 * h - 2 - 2 * m), a1 = gload_pair(xs + 3 * h + 2 * m);
                        const V d2 = gload_pair(xs + h - 2 - 2 * m), a2 = gload_pair(xs + h + 2 * m);
                        const V wd1 = gload_pair(win + 3 * h - 2 - 2 * m), wa1 = gload_pair(win + 3 * h + 2 * m);
                        const V wd2 = gload_pair(win + h - 2 - 2 * m), wa2 = gload_pair(win + h + 2 * m);
                        a = {-(wd1.y * d1.y) - wa1.x * a1.x, -(wd1.x * d1.x) - wa1.y * a1.y};  // u[2m], u[2m+1]
                        b = {wd2.x * d2.x - wa2.y * a2.y, wd2.y * d2.y - wa2.x * a2.x};        // u[M-2-2m], u[M-1-2m]
                    } else {
                        auto y = [&](int j) -> T {  // windowed sample j of the frame; zeros beyond the ends: no load at all
                            const long long i = s0 + j;
                            return (i < 0 || i > (long long)len - 1) ? (T)0 : win[j] * xe[i];
                        };
                        auto u = [&](int i) -> T {
                            return i < h ? -y(3 * h - 1 - i) - y(3 * h + i) : y(i - h) - y(3 * h - 1 - i);
                        };
                        a = {u(2 * m), u(2 * m + 1)};
                        b = {u(NN - 2 - 2 * m), u(NN - 1 - 2 * m)};
                    }
                } else {
                    const T* row = (const T*)p.in + (row0 + c) * NN;
                    a = gload_pair(row + 2 * m);
                    b = gload_pair(row + NN - 2 - 2 * m);
                    if constexpr (C::DST) {  // the odd samples x[2m+1] and x[n-1-2m], negated
                        a.y = -a.y;
                        b.y = -b.y;
                    }
                }
                const V w0 = pw[m], w1 = pw[C::N - 1 - m];
                lds[lds_index<C, -1>(c, m)] = {w0.x * a.x - w0.y * b.y, w0.x * b.y + w0.y * a.x};
                if (2 * m != C::N - 1)
                    lds[lds_index<C, -1>(c, C::N - 1 - m)] = {w1.x * b.x - w1.y * a.y, w1.x * a.y + w1.y * b.x};
            }
            __syncthreads();
        } else if constexpr (C::OLS) {
            // (signal, block) of the tile's first row once, uniform; a row further on wraps into the signals that follow.
            // Packed element m of block fr: the samples st + 2 m and st + 2 m + 1 of its signal, st = s0 + fr S
            const int F = p.ols_blocks, S = p.ols_step, len = p.conv_len;
            const long long r0 = base / C::N, b0 = r0 / F;
            const int fr0 = (int)(r0 - b0 * F);
            using ST = typename C::IT;  // (the storage type of x and the gates: TileCfg::CONV)
            const ST* x0 = (const ST*)p.in + b0 * len;
            const ST* g0 = (C::GATE & 1) ? (const ST*)p.gate_in + b0 * len : x0;  // (the gate of the same signal row; else unused)
            for (int f = tid; f < nv * C::N; f += C::THREADS) {
                const int c = f / C::N, m = f - c * C::N;
                int fr = fr0 + c, db = 0;
                if (fr >= F) {
                    db = fr / F;
                    fr -= db * F;
                }
                const ST* xe = x0 + (long long)db * len;
                const ST* ge = g0 + (long long)db * len;
                const int i = p.ols_start + fr * S + 2 * m;  // (-2N < s0 + fr S < T <= 2^30: 32 bits hold it)
                V x = {(T)0, (T)0};
                if (i >= 0 && i + 1 < len) {
                    x = sload_pair<T>(xe + i);
                    if constexpr (C::GATE & 1) {
                        const V g = sload_pair<T>(ge + i);
                        x = {g.x * x.x, g.y * x.y};
                    }
                } else {  // (zeros beyond the ends: no load at all, of x or of its gate)
                    if (i >= 0 && i < len) {
                        x.x = sload<T>(xe + i);
                        if constexpr (C::GATE & 1) x.x = sload<T>(ge + i) * x.x;
                    }
                    if (i + 1 >= 0 && i + 1 < len) {
                        x.y = sload<T>(&xe[i + 1]);
                        if constexpr (C::GATE & 1) x.y = sload<T>(&ge[i + 1]) * x.y;
                    }
                }
                lds[lds_index<C, -1>(c, m)] = x;
            }
            __syncthreads();
        } else if constexpr (C::CONV) {
            // packed element m of row c: the reals 2 m and 2 m + 1 of a row of L samples, zeros from sample L on
            const int L = p.conv_len;
            using ST = typename C::IT;  // (the storage type of x and the gates: TileCfg::CONV)
            const ST* x0 = (const ST*)p.in + (base / C::N) * L;
            const ST* g0 = (C::GATE & 1) ? (const ST*)p.gate_in + (base / C::N) * L : x0;  // (else unused)
            for (int f = tid; f < nv * C::N; f += C::THREADS) {
                const int c = f / C::N, m = f - c * C::N;
                const ST* xr = x0 + (long long)c * L;
                const ST* gr = g0 + (long long)c * L;
                V x = {(T)0, (T)0};
                if (2 * m + 1 < L) {
                    x = sload_pair<T>(xr + 2 * m);
                    if constexpr (C::GATE & 1) {
                        const V g = sload_pair<T>(gr + 2 * m);
                        x = {g.x * x.x, g.y * x.y};
                    }
                } else if (2 * m < L) {
                    x.x = sload<T>(xr + 2 * m);
                    if constexpr (C::GATE & 1) x.x = sload<T>(gr + 2 * m) * x.x;
                }
                lds[lds_index<C, -1>(c, m)] = x;
            }
            __syncthreads();
        } else if constexpr (C::STFT) {
            // (b, frame) of the tile's first row once, uniform; a row further on wraps into the entries that follow
            const long long r0 = base / C::N, b0 = r0 / p.stft_frames;
            const int fr0 = (int)(r0 - b0 * p.stft_frames);
            const int F = p.stft_frames, hop = p.stft_hop, len = p.stft_len, mode = p.stft_center;
            const int last_start = len - 2 * C::N;  // the last sample a frame may start at and stay inside its entry
            const T* x0 = (const T*)p.in + b0 * len;
            const V* win = (const V*)p.stft_win;
            for (int f = tid; f < nv * C::N; f += C::THREADS) {
                const int c = f / C::N, m = f - c * C::N;
                int fr = fr0 + c, db = 0;
                if (fr >= F) {
                    db = fr / F;
                    fr -= db * F;
                }
                const T* xe = x0 + (long long)db * len;
                const int s0 = fr * hop - (mode ? C::N : 0);  // (fr * hop <= len, or with IADJ < the 2^26 padded samples of istft_adj_check: 32 bits hold it)
                V x;
                if constexpr (C::IADJ) {  // gy / envelope inside [0, len), a selected zero outside: neither is loaded there
                    const T* env = (const T*)p.istft_env + (long long)fr * hop + 2 * m;  // (padded position u = fr hop + j)
                    if (s0 >= 0 && s0 <= last_start) {
                        const V e = gload_pair(env);
                        x = gload_pair(xe + s0 + 2 * m);
                        x = {x.x * e.x, x.y * e.y};
                    } else {
                        T v[2];
#pragma unroll
                        for (int q = 0; q < 2; ++q) {
                            const long long i = (long long)s0 + 2 * m + q;
                            v[q] = (T)0;
                            if (i >= 0 && i < len) v[q] = xe[i] * env[q];
                        }
                        x = {v[0], v[1]};
                    }
                } else if (s0 >= 0 && s0 <= last_start) {
                    x = gload_pair(xe + s0 + 2 * m);
                } else {
                    T v[2];
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        long long i = (long long)s0 + 2 * m + q;
                        const bool outside = i < 0 || i > len - 1;
                        if (i < 0) i = -i;
                        if (i > len - 1) i = 2 * ((long long)len - 1) - i;
                        v[q] = (T)0;
                        if (!outside || mode == 1) v[q] = xe[i];  // (zeros beyond the ends: no load at all)
                    }
                    x = {v[0], v[1]};
                }
                const V w = win[m];
                lds[lds_index<C, -1>(c, m)] = {x.x * w.x, x.y * w.y};
            }
            __syncthreads();
        } else if constexpr (!C::FIRST_DIRECT) {
            // flat, fully coalesced HBM -> LDS copy of the tile (rows need not be 16-B aligned: N = 93)
            const V* gin = (const V*)p.in;
            const int total = nv * C::N;
            {
                for (int f = tid; f < total; f += C::THREADS) {
                    const int c = f / C::N, n = f - c * C::N;
                    V x = {(T)0, (T)0};
                    if constexpr (!same_t<typename C::IT, T>::value)
                        x = load_foreign<C>(p.in, base + f);
                    else if constexpr (C::IN_REAL)
                        x.x = gload_real<(C::NT & 1) != 0>((const T*)p.in + base + f);
                    else
                        x = gload<(C::NT & 1) != 0>(gin + base + f);
                    if (p.inverse && C::CONJ_IN) x.y = -x.y;
                    lds[lds_index<C, -1>(c, n)] = x;
                }
            }
            __syncthreads();
        }
        MIFFT_STAMP(C, 0);  // tile bookkeeping + issue of the next tile's prefetch
        run_pass<C, 0>(p, lds, twr, cur, base, nv, tid, obase, fs_row, drain, slice);
        if constexpr (C::TSTORE) {
            // transposed + twiddled flat store: out[o][c0 + c][k1] = tile[k1][c] * W^{k1 * (c0 + c)}
            const long long o = tt / p.tiles_per_outer;
            const long long c0 = (tt - o * p.tiles_per_outer) * C::TILE;
            V* gout = (V*)p.out + o * (long long)C::N * p.inner + c0 * (long long)C::N;
            const V* tlo = (const V*)p.tlo;
            const V* thi = (const V*)p.thi;
            if constexpr (C::N % C::THREADS == 0 || C::THREADS % C::N == 0) {
                // a thread keeps its k1 for the whole tile: W^(k1 * (c0 + c)) = W^(k1 * c0) [two-level lookup, once
                // per k1] * W^(k1 * c) [plan-time table, read contiguously along k1]
                constexpr int KPT = C::N >= C::THREADS ? C::N / C::THREADS : 1;
                constexpr int CSTEP = C::N >= C::THREADS ? 1 : C::THREADS / C::N;
                const int k1b = C::N >= C::THREADS ? tid : tid % C::N;
                const int cb = C::N >= C::THREADS ? 0 : tid / C::N;
                const V* tcol = (const V*)p.tcol;
                V a[KPT];
#pragma unroll
                for (int kk = 0; kk < KPT; ++kk) {
                    const long long m0 = (long long)(k1b + kk * C::THREADS) * c0;  // < N * inner
                    a[kk] = cmul(tlo[m0 & 1023], thi[m0 >> 10]);
                }
                // all table reads of the tile are issued before the first use (the table is L2-resident)
                constexpr int CIT = (C::TILE + CSTEP - 1) / CSTEP;
                V w[CIT][KPT];
                if constexpr (CSTEP == 1 && C::TILE % 4 == 0) {
                    // only rows 1, 2, 3 and 4, 8, 12, ... of the table are read:
                    // W^(k1 * (c0 + 4 q + r)) = [W^(k1 * c0) * W^(k1 * 4 q)] * W^(k1 * r)
                    constexpr int Q = C::TILE / 4;
                    V lo[3][KPT], hi[Q][KPT];
#pragma unroll
                    for (int kk = 0; kk < KPT; ++kk) {
                        const int k1 = k1b + kk * C::THREADS;
#pragma unroll
                        for (int r = 1; r < 4; ++r) lo[r - 1][kk] = tcol[r * C::N + k1];
#pragma unroll
                        for (int q = 1; q < Q; ++q) hi[q][kk] = tcol[4 * q * C::N + k1];
                    }
#pragma unroll
                    for (int kk = 0; kk < KPT; ++kk) {
                        hi[0][kk] = a[kk];
#pragma unroll
                        for (int q = 1; q < Q; ++q) hi[q][kk] = cmul(a[kk], hi[q][kk]);
#pragma unroll
                        for (int i = 0; i < CIT; ++i)
                            w[i][kk] = (i % 4 == 0) ? hi[i / 4][kk] : cmul(hi[i / 4][kk], lo[i % 4 - 1][kk]);
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < CIT; ++i) {
                        const int c = cb + i * CSTEP;
                        const int cc = c < C::TILE ? c : C::TILE - 1;
#pragma unroll
                        for (int kk = 0; kk < KPT; ++kk) w[i][kk] = cmul(a[kk], tcol[cc * C::N + k1b + kk * C::THREADS]);
                    }
                }
#pragma unroll
                for (int i = 0; i < CIT; ++i) {
                    const int c = cb + i * CSTEP;
                    if (c < nv) {
#pragma unroll
                        for (int kk = 0; kk < KPT; ++kk) {
                            const int k1 = k1b + kk * C::THREADS;
                            V y = cmul(lds[k1 * C::CPITCH + c], w[i][kk]);
                            if (p.inverse) {  // conj(F(conj x)) * conj(W) * 1/N = conj(F(conj x) * W) * 1/N
                                y.x *= (T)p.scale;
                                y.y *= -(T)p.scale;
                            }
                            gstore<(C::NT & 2) != 0>(gout + c * C::N + k1, y);
                        }
                    }
                }
            } else {
                const int total = nv * C::N;
                for (int f = tid; f < total; f += C::THREADS) {
                    const int c = f / C::N, k1 = f - c * C::N;
                    const long long m = (long long)k1 * (c0 + c);  // < N * inner
                    V y = cmul(lds[k1 * C::CPITCH + c], cmul(tlo[m & 1023], thi[m >> 10]));
                    if (p.inverse) {
                        y.x *= (T)p.scale;
                        y.y *= -(T)p.scale;
                    }
                    gstore<(C::NT & 2) != 0>(gout + f, y);
                }
            }
            __syncthreads();
        } else if constexpr (!C::LAST_DIRECT && C::COLS) {
            // a strided PRIME length (one cooperative pass, result in LDS) or a paired-column DCT-II: runs of TILE adjacent columns
            static_assert(C::BIGP(C::NP - 1) || C::DCT == 2, "column tiles store directly unless the last pass works in LDS");
            V* gout = (V*)p.out;
            // DCT = 2: one item per pair of rows (k, N - k), k = 0 .. N / 2, and column; else one per element
            constexpr int SROWS = (C::DCT == 2) ? C::N / 2 + 1 : C::N;
            for (int f = tid; f < SROWS * C::TILE; f += C::THREADS) {
                const int n = f / C::TILE, c = f - n * C::TILE;
                if constexpr (C::DCT == 2) {
                    // V_a = (Z[k] + conj Z[N-k]) / 2 and V_b = (Z[k] - conj Z[N-k]) / 2i are the transforms of the two real
                    // columns; t = W_4n^k V gives X[k] = s Re t and X[N-k] = -s Im t for each
                    if (c < nv) {
                        const V zk = lds[lds_index<C, C::NP - 1>(c, n)], zm = lds[lds_index<C, C::NP - 1>(c, n ? C::N - n : 0)];
                        const T ax = (T)0.5 * (zk.x + zm.x), ay = (T)0.5 * (zk.y - zm.y);
                        const T bx = (T)0.5 * (zk.y + zm.y), by = (T)-0.5 * (zk.x - zm.x);
                        const V w = ((const V*)p.dct_tw)[n];
                        const T s1 = (T)p.dct_s1, sk = n == 0 ? (T)p.dct_s0 : s1;
                        // (DST: bin j of the cosine transform goes to row N - 1 - j)
                        gstore<(C::NT & 2) != 0>(gout + gaddr<C>(p, base, c, C::DST ? C::N - 1 - n : n),
                                                 V{sk * (w.x * ax - w.y * ay), sk * (w.x * bx - w.y * by)});
                        if (n != 0 && 2 * n != C::N)
                            gstore<(C::NT & 2) != 0>(gout + gaddr<C>(p, base, c, C::DST ? n - 1 : C::N - n),
                                                     V{-s1 * (w.x * ay + w.y * ax), -s1 * (w.x * by + w.y * bx)});
                    }
                    continue;
                }
                if (c < nv && (!C::HS || n <= p.store_lim)) {
                    V y = lds[lds_index<C, C::NP - 1>(c, n)];
                    if (p.inverse) {
                        y.x *= (T)p.scale;
                        y.y *= -(T)p.scale;
                    }
                    gout[gaddr<C>(p, base, c, n)] = y;
                }
            }
            __syncthreads();
        } else if constexpr (C::CONV) {
            // Z = F(z) of the packed rows lies in LDS.  One work item per pair (k, N - k), k = 0 .. N / 2, a fixed number per
            // thread in groups of G whose filter loads are all issued before the first product (as the C2R load's)
            const V* w = (const V*)p.r2c_tw;
            constexpr int PAIRS = C::N / 2 + 1;
            constexpr int IT = (C::TILE * PAIRS + C::THREADS - 1) / C::THREADS, G = IT < 4 ? IT : 4;
            const long long row0 = base / C::N;
            const unsigned D = (unsigned)p.conv_D;
            // OLS: the filter row follows the signal row0 / F, and row c of the tile lies (ofr0 + c) / F signals further on
            const unsigned OF = C::OLS ? (unsigned)p.ols_blocks : 1u;
            const long long sig0 = C::OLS ? row0 / (long long)OF : row0;
            const unsigned ofr0 = C::OLS ? (unsigned)(row0 - sig0 * (long long)OF) : 0u;
            const unsigned d0 = (unsigned)(((long long)p.conv_row0 + sig0) % (long long)D);  // (uniform; d0 + c < 2^31)
            const V* hs = (const V*)p.conv_h;
            const T cj = (p.conv_mode & 1) ? (T)-1 : (T)1;
#pragma unroll 1
            for (int i0 = 0; i0 < IT; i0 += G) {
                V ga[G], gb[G];
#pragma unroll
                for (int j = 0; j < G; ++j) {
                    const int f = tid + (i0 + j) * C::THREADS;
                    if ((IT % G == 0 || i0 + j < IT) && f < nv * PAIRS) {
                        const int c = f / PAIRS, k = f - c * PAIRS;
                        const unsigned dc = C::OLS ? (ofr0 + (unsigned)c) / OF : (unsigned)c;
                        const V* hr = hs + (long long)((d0 + dc) % D) * (C::N + 1);
                        ga[j] = hr[k];
                        gb[j] = hr[C::N - k];  // (k = 0: bin N, the last of the row)
                    }
                }
#pragma unroll
                for (int j = 0; j < G; ++j) {
                    const int f = tid + (i0 + j) * C::THREADS;
                    if ((IT % G == 0 || i0 + j < IT) && f < nv * PAIRS) {
                        const int c = f / PAIRS, k = f - c * PAIRS, m = k ? C::N - k : 0;
                        const int ik = lds_index<C, C::NP - 1>(c, k), im = lds_index<C, C::NP - 1>(c, m);
                        const V zk = lds[ik], zm = lds[im];
                        // X[k] and X[N-k], as the R2C store unpacks them
                        const T ex = (T)0.5 * (zk.x + zm.x), ey = (T)0.5 * (zk.y - zm.y);
                        const T ox = (T)0.5 * (zk.y + zm.y), oy = (T)-0.5 * (zk.x - zm.x);
                        const V wk = w[k];
                        const T tx = wk.x * ox - wk.y * oy, ty = wk.x * oy + wk.y * ox;
                        const V xa = {ex + tx, ey + ty}, xb = {ex - tx, ty - ey};
                        // times G (conjugated: correlation)
                        const V ha = {ga[j].x, cj * ga[j].y}, hb = {gb[j].x, cj * gb[j].y};
                        V a = cmul(xa, ha), b = cmul(xb, hb);
                        if (k == 0) a.y = b.y = (T)0;
                        // the C2R fold: Z[k] = E + i O, Z[N-k] = conj(E) + i conj(O), E = a + conj b, O = (a - conj b) conj(W^k);
                        // written conjugated, so that the forward passes run the inverse as conj(F(conj Z))
                        const T fx = a.x + b.x, fy = a.y - b.y, dx = a.x - b.x, dy = a.y + b.y;
                        const T px = dx * wk.x + dy * wk.y, py = dy * wk.x - dx * wk.y;
                        lds[ik] = {fx - py, -(fy + px)};
                        if (k != 0 && 2 * k != C::N) lds[im] = {fx + py, fy - px};
                    }
                }
            }
            __syncthreads();
            // (pass 0 gathers at lds_index<C, -1>, where the last pass left its results: see TileCfg::CONV)
            run_pass<C, 0>(p, lds, twr, cur, base, nv, tid, obase, fs_row, drain, slice);
            // conj(z) of the packed result, unscaled: sample 2 j is the real part of element j, sample 2 j + 1 minus its
            // imaginary part.  Samples o .. o + Lo - 1 go to a row of Lo reals.
            const int o = p.conv_o, Lo = p.conv_Lo;
            const T s = (T)p.scale;
            using ST = typename C::IT;  // (the storage type of out and the postgate: TileCfg::CONV)
            if constexpr (C::OLS) {
                // sample i of block fr goes to out[b Lo + fr S + i - c] for c <= i < c + S and fr S + i - c < Lo only
                const int F = p.ols_blocks, S = p.ols_step;
                ST* out0 = (ST*)p.out + sig0 * Lo;
                const ST* b0 = (C::GATE & 2) ? (const ST*)p.gate_out + sig0 * Lo : out0;  // (else unused)
                for (int f = tid; f < nv * C::N; f += C::THREADS) {
                    const int c = f / C::N, j = f - c * C::N, u = 2 * j - o;
                    if (u + 1 < 0 || u >= S) continue;
                    int fr = (int)ofr0 + c, db = 0;
                    if (fr >= F) {
                        db = fr / F;
                        fr -= db * F;
                    }
                    const int t = fr * S + u;  // (< Lo + 2N: 32 bits hold it)
                    const bool w0 = u >= 0 && t < Lo, w1 = u + 1 < S && t + 1 < Lo;
                    if (!w0 && !w1) continue;
                    const V v = lds[lds_index<C, C::NP - 1>(c, j)];
                    T y0 = v.x * s, y1 = -(v.y * s);
                    ST* q = out0 + (long long)db * Lo + t;
                    const ST* bq = b0 + (long long)db * Lo + t;
                    if (w0 && w1 && ((unsigned long long)q & (2 * sizeof(ST) - 1)) == 0) {
                        if constexpr (C::GATE & 2) {
                            const V g = sload_pair<T>(bq);
                            y0 = g.x * y0, y1 = g.y * y1;
                        }
                        sstore_pair(q, y0, y1);
                    } else {
                        if (w0) {
                            if constexpr (C::GATE & 2) y0 = sload<T>(bq) * y0;
                            sstore(q, y0);
                        }
                        if (w1) {
                            if constexpr (C::GATE & 2) y1 = sload<T>(bq + 1) * y1;
                            sstore(q + 1, y1);
                        }
                    }
                }
            } else {
                ST* out0 = (ST*)p.out + row0 * Lo;
                const ST* b0 = (C::GATE & 2) ? (const ST*)p.gate_out + row0 * Lo : out0;  // (else unused)
                for (int f = tid; f < nv * C::N; f += C::THREADS) {
                    const int c = f / C::N, j = f - c * C::N, t = 2 * j - o;
                    if (t + 1 < 0 || t >= Lo) continue;
                    const V v = lds[lds_index<C, C::NP - 1>(c, j)];
                    T y0 = v.x * s, y1 = -(v.y * s);
                    ST* q = out0 + (long long)c * Lo + t;
                    const ST* bq = b0 + (long long)c * Lo + t;
                    if (t >= 0 && t + 1 < Lo && ((unsigned long long)q & (2 * sizeof(ST) - 1)) == 0) {
                        if constexpr (C::GATE & 2) {
                            const V g = sload_pair<T>(bq);
                            y0 = g.x * y0, y1 = g.y * y1;
                        }
                        sstore_pair(q, y0, y1);
                    } else {
                        if (t >= 0) {
                            if constexpr (C::GATE & 2) y0 = sload<T>(bq) * y0;
                            sstore(q, y0);
                        }
                        if (t + 1 < Lo) {
                            if constexpr (C::GATE & 2) y1 = sload<T>(bq + 1) * y1;
                            sstore(q + 1, y1);
                        }
                    }
                }
            }
            __syncthreads();
        } else if constexpr (C::R2C) {
            // Z = F(z) of the packed row lies in LDS.  E[k] = (Z[k] + conj Z[N-k]) / 2 and O[k] = (Z[k] - conj Z[N-k]) / 2i are
            // the transforms of the even and the odd samples; X[k] = E[k] + W^k O[k] and X[N-k] = conj(E[k] - W^k O[k]) with
            // W = e^(-2 pi i / 2N); k = 0 gives X[0] and X[N].  One thread per pair (k, N - k), both runs of stores contiguous.
            V* gout = (V*)p.out;
            const V* w = (const V*)p.r2c_tw;
            constexpr int PAIRS = C::N / 2 + 1;
            const long long row0 = base / C::N;
            for (int f = tid; f < nv * PAIRS; f += C::THREADS) {
                const int c = f / PAIRS, k = f - c * PAIRS, m = k ? C::N - k : 0;
                const V zk = lds[lds_index<C, C::NP - 1>(c, k)], zm = lds[lds_index<C, C::NP - 1>(c, m)];
                const T ex = (T)0.5 * (zk.x + zm.x), ey = (T)0.5 * (zk.y - zm.y);
                const T ox = (T)0.5 * (zk.y + zm.y), oy = (T)-0.5 * (zk.x - zm.x);
                const V wk = w[k];
                const T tx = wk.x * ox - wk.y * oy, ty = wk.x * oy + wk.y * ox;
                V a = {ex + tx, ey + ty}, b = {ex - tx, ty - ey};
                if constexpr (C::DCT == 2) {
                    // a = V[k], b = V[N-k]: t = W_4n^k a gives X[k] = 2 Re t and X[n-k] = -2 Im t, u = W_4n^(N-k) b gives
                    // X[N-k] and X[N+k].  Four runs of reals over the lanes, two ascending and two descending.  k = 0: X[n]
                    // does not exist and X[N] comes from Re u alone; 2 k = N: a and b are the same bin.
                    const V* w4 = (const V*)p.dct_tw;
                    const V wa = w4[k], wb = w4[C::N - k];
                    const T s1 = (T)p.dct_s1, s0 = k == 0 ? (T)p.dct_s0 : s1;
                    // DST: X[j] goes to n - 1 - j, so Y[n-1-k] = 2 Re t, Y[k-1] = -2 Im t, Y[N-1+k] = 2 Re u, Y[N-1-k] = -2 Im u:
                    // the runs descending, ascending, ascending, descending
                    T* xrow = (T*)p.out + (row0 + c) * (2 * C::N);
                    constexpr int NN = 2 * C::N;
                    xrow[C::DST ? NN - 1 - k : k] = s0 * (wa.x * a.x - wa.y * a.y);
                    if (k) xrow[C::DST ? k - 1 : NN - k] = -s1 * (wa.x * a.y + wa.y * a.x);
                    if (2 * k != C::N) {
                        xrow[C::DST ? C::N - 1 + k : C::N - k] = s1 * (wb.x * b.x - wb.y * b.y);
                        if (k) xrow[C::DST ? C::N - 1 - k : C::N + k] = -s1 * (wb.x * b.y + wb.y * b.x);
                    }
                    continue;
                }
                if constexpr (C::SPEC != 0) {
                    // |a|^2 and |b|^2, or their square roots: bins k and N - k of the frame (k = 0: bins 0 and N; 2 k = N: one bin)
                    T pa = fma_t(a.y, a.y, a.x * a.x), pb = fma_t(b.y, b.y, b.x * b.x);
                    if constexpr (C::SPEC == 1) {
                        pa = sqrt_t(pa);
                        pb = sqrt_t(pb);
                    }
                    if constexpr (C::FB) {  // in place: this work item is the only reader of slots k and m
                        if (k == 0) {
                            lds[lds_index<C, C::NP - 1>(c, 0)] = {pa, pb};
                        } else {
                            lds[lds_index<C, C::NP - 1>(c, k)].x = pa;
                            if (2 * k != C::N) lds[lds_index<C, C::NP - 1>(c, m)].x = pb;
                        }
                    } else {
                        if constexpr (C::LOG) {
                            pa = spec_log<T>(p, pa);
                            pb = spec_log<T>(p, pb);
                        }
                        T* row = (T*)p.out + (row0 + c) * (C::N + 1);
                        gstore_real<(C::NT & 2) != 0>(row + k, pa);
                        if (2 * k != C::N) gstore_real<(C::NT & 2) != 0>(row + C::N - k, pb);
                    }
                    continue;
                }
                if (p.inverse) {  // the inverse of a real row: conj(X) / 2N
                    a.x *= (T)p.scale;
                    a.y *= -(T)p.scale;
                    b.x *= (T)p.scale;
                    b.y *= -(T)p.scale;
                }
                if constexpr (C::IADJ) {
                    if (k == 0) {  // bins 0 and N: c_k = 1 (the table carries the 2 of the others), imaginary parts exactly 0
                        a = {(T)0.5 * a.x, (T)0};
                        b = {(T)0.5 * b.x, (T)0};
                    }
                }
                V* row = gout + (row0 + c) * p.half_pitch;
                gstore<(C::NT & 2) != 0>(row + k, a);
                if (2 * k != C::N) gstore<(C::NT & 2) != 0>(row + C::N - k, b);
            }
            if constexpr (C::FB) {
                // P of the tile's frames lies in LDS: one work item per (row, band), the bands of a row over adjacent lanes
                __syncthreads();
                const int M = p.spec_bands;
                const T* wt = (const T*)p.spec_wt;
                T* orow = (T*)p.out + row0 * M;
                for (int f = tid; f < nv * M; f += C::THREADS) {
                    const int c = f / M, mb = f - c * M;
                    const int lo = p.spec_lo[mb], len = p.spec_len[mb];
                    const T* wb = wt + p.spec_off[mb];
                    T acc = (T)0;
                    for (int j = 0; j < len; ++j) {
                        const int bin = lo + j;  // (<= N: bin N is the .y of slot 0)
                        if constexpr (C::POST) {  // the component alone: the other half of the slot may be written meanwhile
                            const T* ldr = (const T*)lds;
                            acc = fma_t(wb[j], bin == C::N ? ldr[2 * lds_index<C, C::NP - 1>(c, 0) + 1]
                                                           : ldr[2 * lds_index<C, C::NP - 1>(c, bin)], acc);
                        } else {
                            const V s = lds[lds_index<C, C::NP - 1>(c, bin == C::N ? 0 : bin)];
                            acc = fma_t(wb[j], bin == C::N ? s.y : s.x, acc);
                        }
                    }
                    if constexpr (C::LOG) acc = spec_log<T>(p, acc);
                    if constexpr (C::POST)
                        ((T*)lds)[2 * lds_index<C, C::NP - 1>(c, 1 + mb) + 1] = acc;  // (M <= N - 1: slots 1 .. N - 1)
                    else
                        gstore_real<(C::NT & 2) != 0>(orow + f, acc);
                }
                if constexpr (C::POST) {
                    // y of the tile's frames lies in the .y halves: one work item per (row, column of post)
                    __syncthreads();
                    const int Q = p.spec_q;
                    const T* pm = (const T*)p.spec_post;
                    const T* ldr = (const T*)lds;
                    T* zrow = (T*)p.out + row0 * Q;
                    for (int f = tid; f < nv * Q; f += C::THREADS) {
                        const int c = f / Q, q = f - c * Q;
                        T z = (T)0;
                        for (int mb = 0; mb < M; ++mb)
                            z = fma_t(pm[mb * Q + q], ldr[2 * lds_index<C, C::NP - 1>(c, 1 + mb) + 1], z);
                        gstore_real<(C::NT & 2) != 0>(zrow + f, z);
                    }
                }
            }
            __syncthreads();
        } else if constexpr (C::ILV > 0) {
            ilv_store<C>(p, lds, base, nv * C::N, tid);
            __syncthreads();
        } else if constexpr (C::ISTFT) {
            // conj(z) of the packed frames lies in LDS: real j of frame r is component j & 1 of element j >> 1 of row r
            // (adjacent lanes read adjacent slots), its sign and the 1 / 2N part of ws
            constexpr int NN = 2 * C::N;
            const int hop = p.stft_hop, len = p.stft_len, cen = p.stft_center ? C::N : 0, f0 = fs_row;
            const bool last = f0 + nv >= p.stft_frames, warm = t < run_begin;
            const int span = (nv - 1) * hop + NN;                        // samples the tile's frames touch, from f0 hop on
            const int done = last ? span : nv * hop;                     // finished here; the rest goes to the carry
            const int ncarry = (f0 == 0 || t == t_first) ? 0 : NN - hop;  // partial sums waiting (a run starts from zero)
            const int u0 = f0 * hop;                                      // (< 2^26, istft_check; ADJ: < T + n < 2^31, stft_adj_check)
            const T* ldr = (const T*)lds;
            T* carry = (T*)(lds + C::ISTFT_OFF);
            const T* ws = (const T*)p.stft_win;
            const T* env = (const T*)p.istft_env;
            T* outb = (T*)p.out + obase * len;
            for (int i0 = 0; i0 < span; i0 += C::THREADS) {
                const int i = i0 + tid;
                T acc = (T)0;
                if (i < span) {
                    if (i < ncarry) acc = carry[i];
                    int r_hi = i / hop;
                    if (r_hi > nv - 1) r_hi = nv - 1;
                    for (int r = i < NN ? 0 : (i - NN) / hop + 1; r <= r_hi; ++r) {
                        const int j = i - r * hop;
                        acc = fma_t(ws[j], ldr[2 * lds_index<C, C::NP - 1>(r, j >> 1) + (j & 1)], acc);
                    }
                }
                if (!last) __syncthreads();  // (uniform) this chunk's carry reads before its carry writes
                if (i < span) {
                    if (i >= done) {
                        carry[i - done] = acc;
                    } else {
                        const int u = u0 + i;
                        if constexpr (C::ADJ != 0) {  // no envelope; the reflected edges beside the entry's own samples
                            if (!warm) {
                                if (u >= cen && u < cen + len) {
                                    outb[u - cen] = acc;
                                } else if (p.stft_center == 1) {
                                    T* edge = (T*)p.adj_edge + obase * NN;  // (2, N) per entry
                                    if (u < cen) edge[u] = acc;
                                    else if (u - cen - len < C::N) edge[C::N + (u - cen - len)] = acc;
                                }
                            }
                        } else {
                            if (!warm && u >= cen && u < cen + len) outb[u - cen] = acc * env[u];
                        }
                    }
                }
            }
            __syncthreads();
        } else if constexpr (C::DCT == 3 && !C::COLS) {
            // conj(z) of the packed row z_j = v[2j] + i v[2j+1] lies in LDS, already scaled: x[2j] is slot j of v, x[2j+1]
            // slot n - 1 - j; stored as one flat run
            if constexpr (C::DCT_QUADS) {  // quad e of a row from conj z_e and conj z_(N-1-e)
                constexpr int H = C::N / 2;
                for (int f = tid; f < nv * H; f += C::THREADS) {
                    const int c = f / H, e = f - c * H;
                    const V a = lds[lds_index<C, C::NP - 1>(c, e)], b = lds[lds_index<C, C::NP - 1>(c, C::N - 1 - e)];
                    if constexpr (C::DST)  // the odd samples x[4e+1] and x[4e+3], negated
                        gstore4<(C::NT & 2) != 0>((T*)p.out + 2 * base + 4 * (long long)f, a.x, b.y, -a.y, -b.x);
                    else
                        gstore4<(C::NT & 2) != 0>((T*)p.out + 2 * base + 4 * (long long)f, a.x, -b.y, -a.y, b.x);
                }
            } else {
                const T* ldr = (const T*)lds;
                for (int f = tid; f < nv * C::N; f += C::THREADS) {
                    const int c = f / C::N, j = f - c * C::N, q = 2 * C::N - 1 - j;
                    const T x0 = ldr[2 * lds_index<C, C::NP - 1>(c, j >> 1) + (j & 1)];
                    const T x1 = ldr[2 * lds_index<C, C::NP - 1>(c, q >> 1) + (q & 1)];
                    // (DST: the odd sample x[2f+1], negated)
                    gstore<(C::NT & 2) != 0>((V*)p.out + base + f, V{(j & 1) ? -x0 : x0, ((q & 1) != 0) != C::DST ? -x1 : x1});
                }
            }
            __syncthreads();
        } else if constexpr (C::IMDCT) {
            // Z = F(p . z) lies in LDS.  Sweep: element k of every row becomes c_k = p_k Z_k, so slot a of v is the real part
            // of element a / 2 (a even) or minus the imaginary part of element (M - 1 - a) / 2 (a odd)
            constexpr int H = C::N, M = 2 * C::N;
            const V* pw = (const V*)p.dct_tw;
            for (int f = tid; f < nv * H; f += C::THREADS) {
                const int c = f / H, k = f - c * H, at = lds_index<C, C::NP - 1>(c, k);
                const V z = lds[at], w = pw[k];
                lds[at] = {w.x * z.x - w.y * z.y, w.x * z.y + w.y * z.x};
            }
            __syncthreads();
            const int f0 = fs_row, len = p.stft_len;
            const bool last = f0 + nv >= p.stft_frames, warm = t < run_begin;
            const T* ldr = (const T*)lds;
            T* carry = (T*)(lds + C::IMDCT_OFF);
            auto v_at = [&](int c, int a) -> T {
                return (a & 1) ? -ldr[2 * lds_index<C, C::NP - 1>(c, (M - 1 - a) >> 1) + 1] : ldr[2 * lds_index<C, C::NP - 1>(c, a >> 1)];
            };
            if (!warm) {
                // blocks f0 - 1 .. f0 + nv - 2 of the entry: the later frame of block f0 + c - 1 is row c, the earlier one row
                // c - 1 or, for c = 0, the carry; frame 0 of an entry is nobody's later frame
                const int c_lo = f0 == 0 ? 1 : 0;
                const T* ws = (const T*)p.stft_win;
                T* outb = (T*)p.out + obase * len;
                auto sample = [&](int c, int i) -> T {
                    const int a = i < H ? H - 1 - i : i - H;  // y_q[M + i] = -v_q[a]
                    const T e = c == 0 ? carry[a] : v_at(c - 1, a);
                    const T l = i < H ? v_at(c, H + i) : -v_at(c, 3 * H - 1 - i);  // y_(q+1)[i]
                    return fma_t(ws[i], l, ws[M + i] * -e);
                };
                for (int f = tid; f < (nv - c_lo) * H; f += C::THREADS) {
                    const int cc = f / H, i = 2 * (f - cc * H), c = cc + c_lo;
                    const long long o = (long long)(f0 + c - 1) * M + i;
                    if (o + 1 < len) {
                        gstore_pair(outb + o, sample(c, i), sample(c, i + 1));
                    } else if (o < len) {
                        outb[o] = sample(c, i);
                    }
                }
            }
            __syncthreads();  // (uniform) every read of the previous carry before the next one is written
            if (!last)
                for (int a = tid; a < H; a += C::THREADS) carry[a] = v_at(nv - 1, a);
            __syncthreads();
        } else if constexpr (C::DCT == 4) {
            // Z = F(p . z) lies in LDS: item (c, k), k < ceil(N / 2), holds c_k = p_k Z_k and c_(N-1-k) and stores the pairs
            // (X[2k], X[2k+1]) and (X[n-2-2k], X[n-1-2k]) of row c, one run ascending over the lanes and one descending
            constexpr int H2 = (C::N + 1) / 2, NN = 2 * C::N;
            const V* pw = (const V*)p.dct_tw;
            const long long row0 = base / C::N;
            const T s = (T)p.dct_s1;
            for (int f = tid; f < nv * H2; f += C::THREADS) {
                const int c = f / H2, k = f - c * H2;
                const V z0 = lds[lds_index<C, C::NP - 1>(c, k)], z1 = lds[lds_index<C, C::NP - 1>(c, C::N - 1 - k)];
                const V w0 = pw[k], w1 = pw[C::N - 1 - k];
                const T re0 = w0.x * z0.x - w0.y * z0.y, im0 = w0.x * z0.y + w0.y * z0.x;
                const T re1 = w1.x * z1.x - w1.y * z1.y, im1 = w1.x * z1.y + w1.y * z1.x;
                T* row = (T*)p.out + (row0 + c) * NN;
                if constexpr (C::DST) {  // out[2k] = -s Im c_k, out[n-1-2k] = s Re c_k: the same pairs, the roles exchanged
                    gstore_pair(row + 2 * k, -s * im0, s * re1);
                    if (2 * k != C::N - 1) gstore_pair(row + NN - 2 - 2 * k, -s * im1, s * re0);
                } else {
                    gstore_pair(row + 2 * k, s * re0, -s * im1);
                    if (2 * k != C::N - 1) gstore_pair(row + NN - 2 - 2 * k, s * re1, -s * im0);
                }
            }
            __syncthreads();
        } else if constexpr (!C::LAST_DIRECT) {
            V* gout = (V*)p.out;
            const int total = nv * C::N;
            for (int f = tid; f < total; f += C::THREADS) {
                const int c = f / C::N, n = f - c * C::N;
                if (C::HS && n > p.store_lim) continue;
                V y = lds[lds_index<C, C::NP - 1>(c, n)];
                if (p.inverse) {
                    y.x *= (T)p.scale;
                    y.y *= -(T)p.scale;
                }
                gstore<(C::NT & 2) != 0>(gout + base + f, y);
            }
            __syncthreads();
        }
    }
    MIFFT_STAMP_DUMP(C, p);
}


// ---------------------------------------------------------------------------------------------
// plane_kernel<CR, CC>: the two innermost dimensions (N1 x N2, N2 contiguous) of one 2-D slice are
// transformed inside ONE LDS tile: the rows (length N2) by the ROWS configuration CR -- pass 0 straight
// from HBM, last pass left in LDS in natural order -- then the columns (length N1, LDS stride N2) by
// the COLS configuration CC, whose last pass stores straight to HBM along the contiguous axis.
// One HBM read + one HBM write for two dimensions; the reference spends a row kernel, a transpose
// kernel, a row kernel and a transpose back (fft/fft/_ndim_fft_gpu.mojo:634-642).
// Requirements: CR::N == CC::TILE (= N2), CR::TILE == CC::N (= N1), CR::LD == N2, equal thread counts,
// identical LDS twiddle tables (N1 == N2 with the same radices).
// ---------------------------------------------------------------------------------------------
template <class CR, class CC>
__global__ __launch_bounds__(CR::THREADS, CR::MINW) void plane_kernel(const TileParams p) {
    using T = typename CR::T;
    using V = cpx<T>;
    static_assert(!CR::COLS && CC::COLS, "rows configuration first, columns configuration second");
    static_assert(CR::N == CC::TILE && CR::TILE == CC::N && CR::LD == CR::N, "plane geometry");
    static_assert(CR::THREADS == CC::THREADS, "one thread count");
    static_assert(CR::FIRST_DIRECT && !CR::LAST_DIRECT && !CC::FIRST_DIRECT && CC::LAST_DIRECT, "plane data flow");
    static_assert(CR::TWMODE == TW_LDS && CC::TWMODE == TW_LDS, "planes keep their twiddles in LDS");
    // square planes with the same radices share one LDS twiddle table; rectangular planes keep the column table (W_N1,
    // from p.tlo) right behind the row table (W_N2, from p.tw)
    constexpr bool SHARED_TW = CR::N == CC::N && CR::NP == CC::NP && CR::R(0) == CC::R(0) && CR::R(1) == CC::R(1) &&
                               CR::R(2) == CC::R(2) && CR::R(3) == CC::R(3);
    constexpr int CSHIFT = SHARED_TW ? 0 : CR::TWL_TOTAL;
    constexpr size_t PLANE_LDS = (size_t)(CR::DATA_ELEMS + CSHIFT + CC::TWL_TOTAL) * sizeof(V);
    static_assert(CR::DATA_ELEMS == CC::DATA_ELEMS && PLANE_LDS <= 160 * 1024, "plane + twiddle tables must fit LDS");
#ifdef MIFFT_STATIC_LDS
    __shared__ __attribute__((aligned(16))) unsigned char smem[PLANE_LDS];
#else
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
#endif
    V* lds = (V*)smem;
    const int tid0 = threadIdx.x;
    V twr[1];
    fill_lds_tw<CR, 1>(lds + CR::DATA_ELEMS, (const V*)p.tw, tid0, p.inverse);
    if constexpr (!SHARED_TW) fill_lds_tw<CC, 1>(lds + CR::DATA_ELEMS + CSHIFT, (const V*)p.tlo, tid0, p.inverse);
    __syncthreads();

    constexpr long long PLANE = (long long)CR::N * CR::TILE;
    V pre[CR::PREFETCH ? CR::IPT(0) : 1][CR::R(0)];
    long long t = blockIdx.x;
    if constexpr (CR::PREFETCH) {
        if (t < p.n_tiles) load_pass0<CR>(p, pre, tile_id(p, t) * PLANE, CR::TILE, tid0);
    }
    const int tid_entry = tid0;
    for (; t < p.n_tiles; t += gridDim.x) {
        int tid = tid_entry;  // opaque per plane: see tile_kernel
#ifndef MIFFT_NO_OPAQUE_TID
        asm volatile("" : "+v"(tid));
#endif
        const long long base = tile_id(p, t) * PLANE;
        V cur[CR::PREFETCH ? CR::IPT(0) : 1][CR::R(0)];
        if constexpr (CR::PREFETCH) {
#pragma unroll
            for (int k = 0; k < CR::IPT(0); ++k)
#pragma unroll
                for (int j = 0; j < CR::R(0); ++j) cur[k][j] = pre[k][j];
            const long long tn = t + gridDim.x;
            if (tn < p.n_tiles) load_pass0<CR>(p, pre, tile_id(p, tn) * PLANE, CR::TILE, tid);
        }
        auto drain = [&]() {  // before the column side's HBM stores: see tile_kernel / run_pass
            if constexpr (CR::PREFETCH) vm_drain();
        };
        run_pass<CR, 0>(p, lds, twr, cur, base, CR::TILE, tid);  // rows: HBM -> ... -> LDS (natural order)
        V none[1][CC::R(0)];
        run_pass<CC, 0, CSHIFT>(p, lds, twr, none, base, CC::TILE, tid, 0, 0, drain);  // columns: LDS -> ... -> HBM
    }
}

// ---------------------------------------------------------------------------------------------
// plane_kernel_wp<CR, CC, PAD>: the fused plane with WAVE-PRIVATE exchanges.  plane_kernel above flattens the work items
// of every pass over the whole workgroup, so each of its six LDS exchanges needs two workgroup barriers and all 16 waves
// move through load / butterfly / LDS phases in lockstep (measured on 1280 planes of 128 x 128: VALU 24 % busy, LDS 22 %,
// HBM 55 %; removing the barriers -- wrong results, timing only -- saves 11-15 %).  Here a wave OWNS whole transforms:
//   row phase    wave w transforms rows [w*RPW, (w+1)*RPW) through all row passes; the exchanges between its passes touch
//                only its own rows of the LDS plane, and LDS instructions of one wave execute in order, so no barrier
//   hand-over    ONE workgroup barrier (rows complete -> columns may start)
//   column phase wave w transforms columns [w*CPW, (w+1)*CPW) through all column passes, again without a barrier; the last
//                pass stores to HBM (runs of CPW elements per row)
//   a second barrier after the last LDS read of the plane protects the plane buffer against the next plane's first write.
// Two barriers per plane instead of twelve, and the waves drift apart, so one wave's butterflies overlap another's LDS
// and HBM traffic.  LDS pitch N2 + PAD (PAD = 8 elements: four consecutive rows of a CPW-column block fall into four
// different 64-byte bank groups).  Row-phase exchanges keep the XOR swizzle of the rows configuration.
// Requirements: the configurations of plane_kernel; N1 % WAVES == 0, N2 % WAVES == 0, CPW a power of two <= 64, every pass
// an exact number of wave rounds.
// ---------------------------------------------------------------------------------------------
template <class CR, class CC, int PAD_>
struct WavePlane {
    static constexpr int N2 = CR::N, N1 = CC::N, THREADS = CR::THREADS, WAVES = THREADS / 64;
    static constexpr int RPW = N1 / WAVES, CPW = N2 / WAVES, BPL = 64 / (CPW > 0 ? CPW : 1);
    static constexpr int PITCH = N2 + PAD_;
    static constexpr int DATA = N1 * PITCH;
    static constexpr bool SHARED_TW = CR::N == CC::N && CR::NP == CC::NP && CR::R(0) == CC::R(0) && CR::R(1) == CC::R(1) &&
                                      CR::R(2) == CC::R(2) && CR::R(3) == CC::R(3);
    static constexpr int CSHIFT = SHARED_TW ? 0 : CR::TWL_TOTAL;
    static constexpr size_t LDS_BYTES = (size_t)(DATA + CSHIFT + CC::TWL_TOTAL) * 2 * sizeof(typename CR::T);
    static constexpr int RIPT(int i) { return RPW * CR::NB(i) / 64; }
    static constexpr int CIPT(int i) { return CC::NB(i) / BPL; }
    static constexpr bool exact() {
        if (THREADS % 64 || N1 % WAVES || N2 % WAVES || CPW < 1 || CPW > 64 || (CPW & (CPW - 1))) return false;
        for (int i = 0; i < CR::NP; ++i)
            if ((RPW * CR::NB(i)) % 64) return false;
        for (int i = 0; i < CC::NP; ++i)
            if (CC::NB(i) % BPL) return false;
        return true;
    }
};

// work item `sub` of a wave in row pass 0 -> (row of the wave rl, butterfly b).  FS (four-step rows, see plane_kernel_wp):
// the rows of the LDS plane are the COLUMNS of the [N2][N1] view of the transform, so adjacent lanes take adjacent rows
// (RPW x 8-byte runs in HBM) instead of adjacent butterflies
template <class CR, class CC, int PAD, bool FS>
MIFFT_DEV void wp_row_item0(int sub, int& rl, int& b) {
    using G = WavePlane<CR, CC, PAD>;
    if constexpr (FS) {
        rl = sub % G::RPW;
        b = sub / G::RPW;
    } else {
        rl = sub / CR::NB(0);
        b = sub - rl * CR::NB(0);
    }
}

template <class CR, class CC, int PAD, int PART = 0, int NPARTS = 1, bool FS = false>
MIFFT_DEV void wp_load_rows(const TileParams& p, cpx<typename CR::T> (*v)[CR::R(0)], long long base, int wave, int lane) {
    using G = WavePlane<CR, CC, PAD>;
    using V = cpx<typename CR::T>;
    using T = typename CR::T;
    constexpr int R = CR::R(0), NB = CR::NB(0), IPT = G::RIPT(0);
    const V* gin = (const V*)p.in;
#pragma unroll
    for (int k = 0; k < IPT; ++k) {
        int rl, b;
        wp_row_item0<CR, CC, PAD, FS>(k * 64 + lane, rl, b);
        if constexpr (FS) {  // element (row rho, column gamma) of the plane = x[gamma * N1 + rho]
            static_assert(!FS || same_t<typename CR::IT, T>::value, "four-step rows: input of the plan's dtype");
            const unsigned off = (unsigned)b * (unsigned)G::N1 + (unsigned)(wave * G::RPW + rl);
#pragma unroll
            for (int j = 0; j < R; ++j) {
                if ((k * R + j) % NPARTS != PART) continue;
                if constexpr (CR::IN_REAL) {
                    v[k][j].x = gload_real<(CR::NT & 1) != 0>((const T*)p.in + base + (long long)j * NB * G::N1 + off);
                    v[k][j].y = (T)0;
                } else {
                    v[k][j] = gload<(CR::NT & 1) != 0>(gin + base + (long long)j * NB * G::N1 + off);
                }
            }
            continue;
        }
        const unsigned off = (unsigned)(wave * G::RPW + rl) * (unsigned)G::N2 + (unsigned)b;
#pragma unroll
        for (int j = 0; j < R; ++j) {
            if ((k * R + j) % NPARTS != PART) continue;  // (compile-time after unrolling)
            if constexpr (!same_t<typename CR::IT, T>::value) {
                v[k][j] = load_foreign<CR>(p.in, base + j * NB + off);
            } else if constexpr (CR::IN_REAL) {  // real tensor promoted in the load (load_pass0)
                v[k][j].x = gload_real<(CR::NT & 1) != 0>((const T*)p.in + base + j * NB + off);
                v[k][j].y = (T)0;
            } else {
                v[k][j] = gload<(CR::NT & 1) != 0>(gin + base + j * NB + off);
            }
        }
    }
}

template <class CR, class CC, int PAD, int I, class Hook, bool FS = false>
MIFFT_DEV void wp_row_passes(const TileParams& p, cpx<typename CR::T>* lds, cpx<typename CR::T> (*pre)[CR::R(0)], int wave,
                             int lane, Hook between) {
    if constexpr (I < CR::NP) {
        using G = WavePlane<CR, CC, PAD>;
        using T = typename CR::T;
        using V = cpx<T>;
        constexpr int R = CR::R(I), P = CR::P(I), NB = CR::NB(I), IPT = G::RIPT(I);
        const V* ltw = lds + G::DATA;
        V v[IPT][R];
#pragma unroll
        for (int k = 0; k < IPT; ++k) {
            int rl, b;
            if constexpr (I == 0) {
                wp_row_item0<CR, CC, PAD, FS>(k * 64 + lane, rl, b);  // as in wp_load_rows
            } else {
                const int sub = k * 64 + lane;
                rl = sub / NB;
                b = sub - rl * NB;
            }
            V* row = lds + (wave * G::RPW + rl) * G::PITCH;
            if constexpr (I == 0) {
#pragma unroll
                for (int j = 0; j < R; ++j) {
                    v[k][j] = pre[k][j];
                    if (p.inverse && !CR::IN_REAL) v[k][j].y = -v[k][j].y;
                }
            } else {
#pragma unroll
                for (int j = 0; j < R; ++j) v[k][j] = row[swz<CR, I - 1>(b + j * NB)];
                const int pp = b % P;
#pragma unroll
                for (int j = 1; j < R; ++j) v[k][j] = cmul(v[k][j], ltw[CR::TWL_OFF(I) + (j - 1) * P + pp]);
            }
        }
        if constexpr (I > 0) wave_lds_fence();  // this wave's reads of the exchange precede its writes below
#pragma unroll
        for (int k = 0; k < IPT; ++k) {
            int rl, b;
            if constexpr (I == 0) {
                wp_row_item0<CR, CC, PAD, FS>(k * 64 + lane, rl, b);
            } else {
                const int sub = k * 64 + lane;
                rl = sub / NB;
                b = sub - rl * NB;
            }
            V* row = lds + (wave * G::RPW + rl) * G::PITCH;
            Dft<R, T, 1>::run(v[k]);
            const int q = b / P, pp = b - q * P, o0 = q * P * R + pp;
#pragma unroll
            for (int s = 0; s < R; ++s) {
                if constexpr (I == CR::NP - 1) {
                    if constexpr (FS) {
                        // four-step twiddle between the two sides: W_M^(rho * kappa), M = N1 * N2, from the two-level
                        // table behind the plane (lo: W_M^l, l < N2; hi: W_M^(N2 h) = W_N1^h, h < N1)
                        const V* fs = lds + G::LDS_BYTES / sizeof(V);
                        const int m = (wave * G::RPW + rl) * (o0 + s * P);
                        v[k][s] = cmul(v[k][s], cmul(fs[m % G::N2], fs[G::N2 + m / G::N2]));
                    }
                    row[o0 + s * P] = v[k][s];  // hand-over layout: natural order
                } else {
                    row[swz<CR, I>(o0 + s * P)] = v[k][s];
                }
            }
        }
        wave_lds_fence();
        if constexpr (I == 0) between(IntC<1>{});
        wp_row_passes<CR, CC, PAD, I + 1, Hook, FS>(p, lds, pre, wave, lane, between);
    }
}

// WL ("wide last"): the LAST column pass is not wave-private.  Behind one more workgroup barrier its butterflies are dealt
// over the whole workgroup with lanes along the contiguous axis, so that a wave's store instruction writes 64 adjacent
// columns of one row (512-byte runs) instead of CPW columns of 64 / CPW rows (64-byte runs at CPW = 8: every 128-byte line
// written half by one wave and half by its neighbour).  Three workgroup barriers per plane instead of two.
template <class CR, class CC, int PAD, int I, class Hook, class Hook2, bool WL = false>
MIFFT_DEV void wp_col_passes(const TileParams& p, cpx<typename CR::T>* lds, long long base, int wave, int lane,
                             Hook before_stores, Hook2 between) {
    if constexpr (WL && I == CC::NP - 1 && I > 0) {
        using G = WavePlane<CR, CC, PAD>;
        using T = typename CR::T;
        using V = cpx<T>;
        constexpr int R = CC::R(I), P = CC::P(I), NB = CC::NB(I);
        static_assert((NB * G::N2) % G::THREADS == 0 && G::THREADS % G::N2 == 0, "whole sweeps of the last column pass");
        constexpr int KPT = NB * G::N2 / G::THREADS, BSTEP = G::THREADS / G::N2;
        const V* ltw = lds + G::DATA + G::CSHIFT;
        const int tid = wave * 64 + lane;
        const int c = tid % G::N2, b0 = tid / G::N2;
        __syncthreads();  // every wave's scatter of pass NP-2 is complete
        V v[KPT][R];
#pragma unroll
        for (int k = 0; k < KPT; ++k) {
            const int b = b0 + k * BSTEP;
#pragma unroll
            for (int j = 0; j < R; ++j) v[k][j] = lds[(b + j * NB) * G::PITCH + c];
            const int pp = b % P;
#pragma unroll
            for (int j = 1; j < R; ++j) v[k][j] = cmul(v[k][j], ltw[CC::TWL_OFF(I) + (j - 1) * P + pp]);
        }
        MIFFT_STAMP(G, 4);
        __syncthreads();  // last LDS read of this plane
        MIFFT_STAMP(G, 5);
        before_stores();
        MIFFT_STAMP(G, 6);
        V* gout = (V*)p.out;
#pragma unroll
        for (int k = 0; k < KPT; ++k) {
            const int b = b0 + k * BSTEP;
            Dft<R, T, 1>::run(v[k]);
            const int q = b / P, pp = b - q * P, o0 = q * P * R + pp;
            const unsigned off = (unsigned)o0 * (unsigned)G::N2 + (unsigned)c;
#pragma unroll
            for (int s = 0; s < R; ++s) {
                if (CC::HS && s * P > CC::N / 2) continue;  // (never stored: not computed either, see pass_compute_scatter)
                V y = v[k][s];
                if (p.inverse) {
                    y.x *= (T)p.scale;
                    y.y *= -(T)p.scale;
                }
                if (!CC::HS || o0 + s * P <= p.store_lim) gstore<(CC::NT & 2) != 0>(gout + base + (long long)s * P * G::N2 + off, y);
            }
        }
    } else if constexpr (I < CC::NP) {
        using G = WavePlane<CR, CC, PAD>;
        using T = typename CR::T;
        using V = cpx<T>;
        constexpr int R = CC::R(I), P = CC::P(I), NB = CC::NB(I), IPT = G::CIPT(I);
        const V* ltw = lds + G::DATA + G::CSHIFT;
        const int cl = lane % G::CPW, bl = lane / G::CPW;
        V* col = lds + wave * G::CPW + cl;
        V v[IPT][R];
#pragma unroll
        for (int k = 0; k < IPT; ++k) {
            const int b = bl + k * G::BPL;
#pragma unroll
            for (int j = 0; j < R; ++j) v[k][j] = col[(b + j * NB) * G::PITCH];
            if constexpr (I > 0) {
                const int pp = b % P;
#pragma unroll
                for (int j = 1; j < R; ++j) v[k][j] = cmul(v[k][j], ltw[CC::TWL_OFF(I) + (j - 1) * P + pp]);
            }
        }
        if constexpr (I == CC::NP - 1) {
            MIFFT_STAMP(G, 4);  // column passes up to the last gather
            __syncthreads();  // last LDS read of this plane: the next plane's row passes may overwrite the buffer
            MIFFT_STAMP(G, 5);  // barrier behind the last gather
            before_stores();  // wait for the prefetched plane ahead of the HBM stores (run_pass)
            MIFFT_STAMP(G, 6);  // drain: wait for the prefetched plane
        } else {
            wave_lds_fence();
        }
        V* gout = (V*)p.out;
#pragma unroll
        for (int k = 0; k < IPT; ++k) {
            const int b = bl + k * G::BPL;
            Dft<R, T, 1>::run(v[k]);
            const int q = b / P, pp = b - q * P, o0 = q * P * R + pp;
            if constexpr (I == CC::NP - 1) {
                const unsigned off = (unsigned)o0 * (unsigned)G::N2 + (unsigned)(wave * G::CPW + cl);
#pragma unroll
                for (int s = 0; s < R; ++s) {
                    if (CC::HS && s * P > CC::N / 2) continue;
                    V y = v[k][s];
                    if (p.inverse) {
                        y.x *= (T)p.scale;
                        y.y *= -(T)p.scale;
                    }
                    if (!CC::HS || o0 + s * P <= p.store_lim)
                        gstore<(CC::NT & 2) != 0>(gout + base + (long long)s * P * G::N2 + off, y);
                }
            } else {
#pragma unroll
                for (int s = 0; s < R; ++s) col[(o0 + s * P) * G::PITCH] = v[k][s];
            }
        }
        if constexpr (I < CC::NP - 1) wave_lds_fence();
        if constexpr (I == 0 && CC::NP > 1) between(IntC<3>{});
        wp_col_passes<CR, CC, PAD, I + 1, Hook, Hook2, WL>(p, lds, base, wave, lane, before_stores, between);
    }
}

// FS = true: the same kernel as a ONE-DIMENSIONAL transform of M = N1 * N2 points per "plane" (four-step inside LDS):
//   X[N2 kr + kc] = sum_rho W_N1^(rho kr) * W_M^(rho kc) * [ sum_gamma x[N1 gamma + rho] W_N2^(gamma kc) ]
// i.e. row rho of the plane holds x[N1 gamma + rho] (the loads transpose: adjacent lanes take adjacent rows), the row side
// transforms over gamma, its last pass multiplies by W_M^(rho kc), the column side transforms over rho and stores the
// result in natural order.  Twiddles of one 128-point side + a two-level table of N1 + N2 entries replace the M-entry
// table a one-row-per-workgroup tile kernel reads from L2 in every pass (p.thi = the M-entry table W_M^m, forward).
template <class CR, class CC, int PAD, bool FS = false, bool WL = false>
__global__ __launch_bounds__(CR::THREADS, CR::MINW) void plane_kernel_wp(const TileParams p) {
    using G = WavePlane<CR, CC, PAD>;
    using T = typename CR::T;
    using V = cpx<T>;
    static_assert(!CR::COLS && CC::COLS && CR::N == CC::TILE && CR::TILE == CC::N, "plane geometry");
    static_assert(CR::THREADS == CC::THREADS && CR::TWMODE == TW_LDS && CC::TWMODE == TW_LDS, "one thread count, LDS twiddles");
    static_assert(G::exact(), "every pass must be an exact number of wave rounds over wave-owned rows / columns");
    static_assert(G::LDS_BYTES <= 160 * 1024, "plane + twiddle tables must fit LDS");
    constexpr size_t FS_BYTES = FS ? (size_t)(G::N1 + G::N2) * sizeof(V) : 0;  // two-level four-step table behind the plane
    static_assert(G::LDS_BYTES + FS_BYTES <= 160 * 1024 && G::LDS_BYTES % sizeof(V) == 0, "four-step table must fit too");
#ifdef MIFFT_STATIC_LDS
    __shared__ __attribute__((aligned(16))) unsigned char smem[G::LDS_BYTES + FS_BYTES];
#else
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
#endif
    V* lds = (V*)smem;
    const int tid0 = threadIdx.x;
    fill_lds_tw<CR, 1>(lds + G::DATA, (const V*)p.tw, tid0, p.inverse);
    if constexpr (!G::SHARED_TW) fill_lds_tw<CC, 1>(lds + G::DATA + G::CSHIFT, (const V*)p.tlo, tid0, p.inverse);
    if constexpr (FS) {
        V* fs = lds + G::LDS_BYTES / sizeof(V);
        const V* wm = (const V*)p.thi;
        for (int e = tid0; e < G::N2 + G::N1; e += CR::THREADS) fs[e] = e < G::N2 ? wm[e] : wm[(e - G::N2) * G::N2];
    }
    __syncthreads();

    constexpr long long PLANE = (long long)G::N1 * G::N2;
    MIFFT_STAMP(G, -1);
    V pre[G::RIPT(0)][CR::R(0)];
    long long t = blockIdx.x;
    if (t < p.n_tiles) wp_load_rows<CR, CC, PAD, 0, 1, FS>(p, pre, tile_id(p, t) * PLANE, tid0 >> 6, tid0 & 63);
    for (; t < p.n_tiles; t += gridDim.x) {
        int tid = tid0;  // opaque per plane: offsets are re-derived instead of being hoisted and kept live (tile_kernel)
#ifndef MIFFT_NO_OPAQUE_TID
        asm volatile("" : "+v"(tid));
#endif
        const int wave = tid >> 6, lane = tid & 63;
        const long long base = tile_id(p, t) * PLANE;
        V cur[G::RIPT(0)][CR::R(0)];
#pragma unroll
        for (int k = 0; k < G::RIPT(0); ++k)
#pragma unroll
            for (int j = 0; j < CR::R(0); ++j) cur[k][j] = pre[k][j];
        const long long tn = t + gridDim.x;
        // the next plane's loads in four slices: here, behind the first row exchange, behind the hand-over barrier and
        // behind the first column exchange (see run_pass: a burst of loads stalls every wave in its issue)
        constexpr int SLICES = (CR::PREFETCH && MIFFT_SLICED_PREFETCH_PLANE) ? 4 : 1;
        const long long nbase = tn < p.n_tiles ? tile_id(p, tn) * PLANE : 0;
        if (CR::PREFETCH && tn < p.n_tiles) wp_load_rows<CR, CC, PAD, 0, SLICES, FS>(p, pre, nbase, wave, lane);
        auto slice = [&](auto kc) {
            constexpr int K = decltype(kc)::value;
            if constexpr (CR::PREFETCH && SLICES > 1 && K >= 1 && K < SLICES) {
                if (tn < p.n_tiles) wp_load_rows<CR, CC, PAD, K, SLICES, FS>(p, pre, nbase, wave, lane);
            }
        };
        auto drain = [&]() {  // ahead of this plane's HBM stores (tile_kernel / run_pass)
            if constexpr (CR::PREFETCH) vm_drain();
        };
        MIFFT_STAMP(G, 0);  // plane bookkeeping, take-over of the prefetched registers, first slice of the next loads
        wp_row_passes<CR, CC, PAD, 0, decltype(slice), FS>(p, lds, cur, wave, lane, slice);
        MIFFT_STAMP(G, 1);  // row passes (wave-private)
        __syncthreads();  // hand-over: every row is complete before any column starts
        MIFFT_STAMP(G, 2);  // hand-over barrier
        slice(IntC<2>{});
        wp_col_passes<CR, CC, PAD, 0, decltype(drain), decltype(slice), WL>(p, lds, base, wave, lane, drain, slice);
        MIFFT_STAMP(G, 3);  // column passes incl. the barrier behind the last gather and the HBM stores
        if (!CR::PREFETCH && tn < p.n_tiles) wp_load_rows<CR, CC, PAD, 0, 1, FS>(p, pre, tile_id(p, tn) * PLANE, wave, lane);
    }
    MIFFT_STAMP_DUMP(G, p);
}

#ifdef MIFFT_EXPERIMENTAL  // lab builds only: a documented negative result (DESIGN_EXPERIMENTS.md), not in libmifft.so
// ---------------------------------------------------------------------------------------------
// image_kernel<CR, CC>: the two innermost dimensions (N1 x N2, N2 contiguous) of images that do NOT fit LDS but fit
// one XCD's 4-MB L2 (100 x 640 x 480: 2.4 MB each).  Every XCD owns whole images: its workgroups transform the rows
// of an image (x -> out, configuration CR), meet at an XCD-LOCAL barrier, and transform the columns in place
// (configuration CC) while the row results are still in that XCD's L2 -- the column pass reads L2 instead of HBM, and
// row results that are overwritten before they are evicted never reach HBM at all (guide: "each XCD has its own L2,
// so make the blockIdx -> tile mapping XCD-aware").
//   * XCD of a workgroup: the hardware XCC_ID register, not an assumption about the dispatch order; the slot inside the
//     XCD is a ticket from an atomic counter that lives in that XCD's L2.
//   * barrier: one arrival counter per XCD, relaxed agent-scope atomics (executed in the L2 all participants share).
//     The stores of a phase are complete in L2 before the arrival is counted (__syncthreads() drains vmcnt); an
//     agent-scope RELEASE fence is deliberately not used -- on gfx942/950 it writes the L2 back to HBM.
//   * every spin is bounded (a dispatch that does not give each XCD its workgroups ends with a wrong result instead of
//     a hang); the host probes the XCC_ID distribution of the same launch geometry at plan time before it selects this
//     kernel (kernels_jit.cpp).
// Launch: 8 * wgs_per_xcd workgroups, all resident (one per CU); counters zeroed before every launch.
// ---------------------------------------------------------------------------------------------
struct ImageParams {
    const void* in;
    void* out;
    const void* tw_rows;  // W_N2
    const void* tw_cols;  // W_N1
    long long n_images;
    unsigned* counters;  // [0..7] tickets, [8..15] arrivals (zeroed before every launch), [16] sticky error flags
    int wgs_per_xcd;
    int inverse;
};

MIFFT_DEV unsigned xcc_id() {
    unsigned v;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(v));
    return v & 0xf;
}

// error flags of the image kernel (ImageParams::counters[16]; read and cleared by mifft_plan_device_status)
enum { IMAGE_ERR_SPIN_EXPIRED = 1u, IMAGE_ERR_SURPLUS_WORKGROUP = 2u };

MIFFT_DEV void xcd_barrier(unsigned* arrive, unsigned target, int tid, unsigned* err) {
    __syncthreads();  // workgroup-scope release: every wave's global stores of the phase are complete in L2
    if (tid == 0) {
        __hip_atomic_fetch_add(arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        unsigned spins = 0;
        while (__hip_atomic_load(arrive, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target && ++spins < (1u << 20))
            __builtin_amdgcn_s_sleep(8);
        // the bounded spin gave up: this workgroup goes on WITHOUT its XCD's row results being complete, so the output
        // of this exec is not to be trusted -- say so where the host can see it
        if (spins >= (1u << 20)) __hip_atomic_fetch_or(err, (unsigned)IMAGE_ERR_SPIN_EXPIRED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // drop this CU's L1 lines; nothing is written back
}

template <class CR, class CC>
__global__ __launch_bounds__(CR::THREADS, 1) void image_kernel(const ImageParams q) {
    using T = typename CR::T;
    using V = cpx<T>;
    static_assert(!CR::COLS && CC::COLS && CR::THREADS == CC::THREADS, "rows configuration, columns configuration");
    static_assert(CR::FIRST_DIRECT && CR::LAST_DIRECT && CC::FIRST_DIRECT && CC::LAST_DIRECT, "direct tiles");
    static_assert(CR::TWMODE == TW_LDS && CC::TWMODE == TW_LDS && !CR::PREFETCH && !CC::PREFETCH, "LDS twiddles");
    static_assert(!CR::BIGP0 && !CC::BIGP0 && !CC::TSTORE, "register butterflies only");
    constexpr int MAXD = CR::DATA_ELEMS > CC::DATA_ELEMS ? CR::DATA_ELEMS : CC::DATA_ELEMS;
    constexpr int TWS_R = MAXD - CR::DATA_ELEMS, TWS_C = MAXD + CR::TWL_TOTAL - CC::DATA_ELEMS;
    constexpr size_t IMAGE_LDS = (size_t)(MAXD + CR::TWL_TOTAL + CC::TWL_TOTAL) * sizeof(V);
    static_assert(IMAGE_LDS <= 160 * 1024, "tiles + both twiddle tables must fit LDS");
    __shared__ __attribute__((aligned(16))) unsigned char smem[IMAGE_LDS];
    __shared__ unsigned s_slot;
    V* lds = (V*)smem;
    const int tid0 = threadIdx.x;
    constexpr long long N1 = CC::N, N2 = CR::N;

    fill_lds_tw<CR, 1>(lds + MAXD, (const V*)q.tw_rows, tid0, q.inverse);
    fill_lds_tw<CC, 1>(lds + MAXD + CR::TWL_TOTAL, (const V*)q.tw_cols, tid0, q.inverse);
    const unsigned xcc = xcc_id() & 7;
    if (tid0 == 0) s_slot = __hip_atomic_fetch_add(q.counters + xcc, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const long long slot = s_slot, W = q.wgs_per_xcd;
    unsigned* arrive = q.counters + 8 + xcc;
    if (slot >= W) {  // more workgroups on this XCD than planned (the plan-time probe rules this out): another XCD is
                      // short of workgroups and its barrier cannot complete -- flag the exec and take no part
        if (tid0 == 0) __hip_atomic_fetch_or(q.counters + 16, (unsigned)IMAGE_ERR_SURPLUS_WORKGROUP, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }

    TileParams pr{}, pc{};
    pr.in = q.in;
    pr.out = q.out;
    pr.tw = q.tw_rows;
    pr.inner = 1;
    pr.inverse = q.inverse;
    pr.scale = q.inverse ? 1.0 / (double)N2 : 1.0;
    pc.in = q.out;
    pc.out = q.out;
    pc.tw = q.tw_cols;
    pc.inner = N2;
    pc.inverse = q.inverse;
    pc.scale = q.inverse ? 1.0 / (double)N1 : 1.0;
    constexpr long long TILES_R = (N1 + CR::TILE - 1) / CR::TILE, TILES_C = (N2 + CC::TILE - 1) / CC::TILE;
    V twr[1];
    V none_r[1][CR::R(0)], none_c[1][CC::R(0)];
    unsigned phase = 0;
    for (long long img = xcc; img < q.n_images; img += 8) {
        const long long ibase = img * N1 * N2;
        for (long long tr = slot; tr < TILES_R; tr += W) {  // rows of this image: x -> out
            int tid = tid0;
            asm volatile("" : "+v"(tid));
            const long long left = N1 - tr * CR::TILE;
            run_pass<CR, 0, TWS_R>(pr, lds, twr, none_r, ibase + tr * CR::TILE * N2, (int)(left < CR::TILE ? left : CR::TILE), tid);
            __syncthreads();
        }
        xcd_barrier(arrive, (unsigned)((++phase) * W), tid0, q.counters + 16);
        for (long long tc = slot; tc < TILES_C; tc += W) {  // columns, in place, from this XCD's L2
            int tid = tid0;
            asm volatile("" : "+v"(tid));
            const long long left = N2 - tc * CC::TILE;
            run_pass<CC, 0, TWS_C>(pc, lds, twr, none_c, ibase + tc * CC::TILE, (int)(left < CC::TILE ? left : CC::TILE), tid);
            __syncthreads();
        }
        // no barrier here: the next image is other memory, and every workgroup still arrives exactly once per barrier
    }
}

#endif  // MIFFT_EXPERIMENTAL

// persistent grid: enough workgroups to fill every CU to its LDS / wave limit.  The formula ignores registers, so a kernel
// that holds fewer workgroups than it launches leaves the surplus waiting for a slot; whether that hurts is kernel by kernel
// (rows480: 4 launched / 3 resident 0.0873 ms, 3 launched 0.0834 ms; rows128: 8 launched / 5 resident is 2-7 % FASTER than
// 5 launched -- the late workgroups fill the holes of the ragged end), so measured per-kernel values override the formula
// (`wg_per_cu_override`, from kGridPerCu in kernels_fast.hip) instead of a general occupancy rule.
template <class C>
inline long long tile_grid(int num_cus, long long n_tiles, int wg_per_cu_override = 0) {
    long long per_cu = (160 * 1024) / (long long)(C::LDS_BYTES ? C::LDS_BYTES : 1);
    const long long wave_limit = 2048 / C::THREADS;
    if (per_cu > wave_limit) per_cu = wave_limit;
    if (per_cu > 8) per_cu = 8;
    if (per_cu < 1) per_cu = 1;
    if (wg_per_cu_override > 0) per_cu = wg_per_cu_override;
    long long grid = (long long)num_cus * per_cu;
    if (grid > n_tiles) grid = n_tiles;
    return grid < 1 ? 1 : grid;
}

}  // namespace mifft
