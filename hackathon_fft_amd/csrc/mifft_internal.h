// mifft_internal.h -- plan structures shared by the C-ABI layer and the kernel
// launchers of libmifft (MI355X / gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mifft.h"
#include "mifft_config.h"

namespace mifft {

// ---- host-only planner (planner.cpp) --------------------------------------
// Independent implementation of the reference's radix planning rules:
//   _times_divisible_by / _build_ordered_bases   fft/fft/_utils.mojo:125-183
//   _get_ordered_bases_processed_list            fft/fft/_utils.mojo:186-221
//   _estimate_best_bases                         fft/fft/fft.mojo:49-104
int plan_ordered_bases(uint64_t length, const std::vector<uint64_t>& user, std::vector<uint32_t>& ordered,
                       std::vector<uint32_t>& processed, std::string& err);
std::vector<uint64_t> plan_estimate_bases(uint64_t length, bool gpu_target);

// ---- error plumbing (mifft_api.cpp) ----------------------------------------
int set_error(int code, const std::string& msg);
int hip_error(hipError_t e, const char* what);
#define MIFFT_HIP_TRY(expr)                                   \
    do {                                                      \
        hipError_t _e = (expr);                               \
        if (_e != hipSuccess) return ::mifft::hip_error(_e, #expr); \
    } while (0)

// ---- plan -------------------------------------------------------------------
struct Plan;
struct DimPass;

// Launches the 1-D transforms of one dimension for `count` leading-batch
// entries.  `in` is x (only for the last dimension, which runs first) or `out`
// itself (in-place tile passes for the strided dimensions).
typedef int (*LaunchFn)(const Plan& plan, const DimPass& pass, const void* in, void* out, int64_t count,
                        hipStream_t stream);

struct DimPass {
    int dim_index = 0;
    int dim_index2 = -1;  // >= 0: a fused plane pass that also transforms this (next-outer) dimension
    int64_t row2d_m = 0;  // > 0: four-step rows inside LDS (plane_kernel_wp<.., FS>): M-entry forward table in d_aux3
    int64_t N1 = 0;       // length of dim_index2
    int64_t N = 0;        // transform length
    int64_t inner = 1;    // element stride of this dim = prod(dims after it)
    int64_t outer = 1;    // prod(dims before it)   (times batch at launch)
    std::vector<uint32_t> radices;    // descending stage radices (reference order)
    std::vector<uint32_t> processed;  // prefix products P_b
    int cfg_np = 0, cfg_r[4] = {1, 1, 1, 1};  // select_fast: the selected table entry's passes and radices (TileCfg NP, R0..R3)
    void* d_twiddle = nullptr;        // device table W_N^n, n in [0,N), complex<out dtype>
    void* d_aux = nullptr;            // kernel-family specific device table (may be null)
    const char* kernel_name = "none";
    LaunchFn launch = nullptr;
    int (*prepare)() = nullptr;  // plan-time, on the plan's device (per-device kernel attributes)
    // geometry chosen by the kernel family at plan time
    int tile = 1;          // transforms per workgroup tile
    int ld = 0;            // LDS leading dimension (complex elements)
    int threads = 256;
    size_t lds_bytes = 0;
    bool first = false;    // reads x (with in_dtype / in_components) instead of out
    // buffer routing of the four-step passes (kernels_fourstep.hip): 0 = x, 1 = out, 2 = plan scratch;
    // -1 = the default (first ? x : out) -> out
    int src_buf = -1, dst_buf = -1;
    int64_t fs_n1 = 0, fs_n2 = 0;  // four-step factors of the dimension (transpose + twiddle pass)
    void* d_aux2 = nullptr;
    bool needs_counters = false;      // image kernel: d_aux2 holds 16 unsigned counters, zeroed before every launch
    bool plane_needs_tw1 = false;     // rectangular fused plane: d_aux holds the W_N1 table of the column side
    void* jit_fn = nullptr;           // runtime-compiled kernel (hipFunction_t) of kernels_jit.cpp passes
    void* d_aux3 = nullptr;           // TSTORE passes: [tile][N] table of W^(c*k1) for the columns of one tile
    bool reverse = false;             // in-place pass that walks its tiles last-to-first (TileParams::reverse)
    int wg_per_cu = 0;                // workgroups per CU of the persistent grid (0 = the LDS / wave-count formula)
    // last pass of a real-input 2-D .. 4-D plan: the kernel families may take a Hermitian twin (TileCfg::HERM) that reads
    // and transforms only the columns up to their mirror.  want_herm is set by the scheduler, herm_d0 / herm_d1 / herm_d2 (the
    // trailing dimensions of the column space) by the family that selected such a kernel (0 = an ordinary kernel).
    bool want_herm = false;
    bool herm_only = false;  // (select_fast: accept only Hermitian twins -- the scheduler tries those first)
    int herm_d0 = 0, herm_d1 = 0, herm_d2 = 0;
    // ... and the half axis of the column space (TileParams::herm_dj ...): size, stride, row length, covered prefix of a row
    int herm_dj = 0, herm_js = 0, herm_L = 0, herm_H = 0;
    // an ordinary column pass between a half-store first pass and the Hermitian last pass transforms only the first
    // col_prefix columns of its column space (0 = all): the others were not stored and are not read
    long long col_prefix = 0;
    bool prefix_ok = false;  // the selected kernel honours col_prefix (the column tiles do, special routes do not)
    // the pass BEFORE such a last pass (it transforms dims[1], the dimension the Hermitian pass halves; a plane: its column
    // side) may store only the results 0 .. store_lim = dims[1] / 2 (TileCfg::HS): want_half asks the families for such a
    // kernel ONLY, `hs` says the selected kernel is one
    bool want_half = false, hs = false;
    bool r2c = false;  // packed real rows (TileCfg::R2C): the kernel runs N / 2 points; d_twiddle is that table, d_aux W_N^k
    bool c2r = false;  // half spectrum -> packed real rows (TileCfg::C2R): the same tables as r2c
    // TileCfg::DCT of a packed-row pass (2: DCT-II on an r2c kernel, 3: its inverse on a c2r one) or of a paired-column pass
    // (neither r2c nor c2r; `inner` counts pairs of real columns): d_aux2 holds W_4N^k, k = 0 .. N / 2; the scales of bin 0
    // and of the other bins (TileParams::dct_s0 / dct_s1)
    // 4 (DCT-IV): neither r2c nor c2r; the kernel runs N / 2 complex points over rows of N reals, d_twiddle is that forward
    // table, d_aux2 holds p_m = e^(-i pi (8m+1) / 8N), m < N / 2, and dct_s1 the one scale.  mdct: the rows are the `outer`
    // lapped frames of every batch entry (TileCfg::MDCT); d_aux3 holds the window, 2 N values of the plan's float type
    int dct = 0;
    bool mdct = false;
    // dst (with dct = 2 / 3 / 4, never with mdct / imdct): TileCfg::DST, the sine transform of that type on the same tile, tables
    // and scales; part of the kernel's configuration and name (`dst2` / `dst3` / `dst4`)
    bool dst = false;
    // imdct: the rows are `outer` frames of N coefficients per batch entry, unfolded and overlap-added into dims[0] samples by
    // the store (TileCfg::IMDCT); d_aux3 holds gain * w, 2 N values of the plan's float type; istft_min_run as below
    bool imdct = false;
    double dct_s0 = 1.0, dct_s1 = 1.0;
    // TileCfg::STFT of a packed-row pass: the rows are the `outer` frames of every batch entry (hop, length and centring are the
    // plan's); d_aux2 holds the window, N values of the plan's float type
    bool stft = false;
    // TileCfg::CONV of a packed-row (r2c) pass: rows of dims[0] samples are convolved with the plan's filter spectra in the one
    // launch (conv.cpp); d_twiddle and d_aux are the r2c tables, N is the FFT length
    bool conv = false;
    // TileCfg::WGRAD beside it: the pass is the filter gradient of that convolution (conv.cpp), launched by launch_jit_conv_grad
    bool wgrad = false;
    // TileCfg::ISTFT of a C2R pass: `outer` frames per batch entry are overlap-added into dims[0] samples; d_aux2 holds the
    // synthesis table (N values), d_aux3 the reciprocal envelope (N + hop (outer - 1) values), both of the plan's float type
    bool istft = false;
    int istft_min_run = 1;  // (Config::istft_min_run when the pass was built: the grid is at most n_tiles / istft_min_run)
    int64_t half_pitch = 0;  // R2C / C2R: row pitch (complex elements) of the half-spectrum side; 0 = N (full-spectrum rows)
    int store_lim = 0;
    bool ilv = false;  // interleaved block tile (TileCfg::ILV): `inner` (< 128 B of elements) transforms per block, launched as rows
    bool regime_twin = false;  // select_fast took an entry tuned for a size regime (non-temporal twin): not to be traded for
                               // a runtime-specialised half-store kernel
};

// The request of a fused FFT convolution plan (a MIFFT_FLAG_STFT plan whose payload starts with MIFFT_CONV_TAG or
// MIFFT_CONV_GRAD_TAG), as conv_check / conv_grad_check decoded it; dims = {L, n}.  x is (batch, L, 1) real, out
// (batch, Lo, 1): the samples o .. o + Lo - 1 of irfft(rfft(x, n) G, n), row r against row r % D of the caller's device
// buffer h (D rows of n / 2 + 1 complex values; never copied, never freed); mode bit 0: G = conj(H).
struct ConvRequest {
    int64_t D = 0, o = 0, Lo = 0;  // (D = 0: the plan is no convolution)
    // overlap-save (S > 0): dims = {T, n}; every row is F blocks of n samples, block f from sample s0 + f S on (zeros outside
    // the row), of whose circular result the S samples from o (= c) on are stored at f S of the row's Lo output samples.
    // A single block has S = 0, F = 1, s0 = 0, in a filter-gradient plan as well.
    int64_t S = 0, F = 1, s0 = 0;
    // partitioned overlap-save (Q > 0): the filter is `parts` partitions of Q taps, h (D, parts, n / 2 + 1) complex values;
    // block f sums, over the partitions p, the block of n samples from s0 + f S - p Q on (correlation: + p Q) times spectrum (d, p)
    int64_t Q = 0, parts = 0;
    // the filter gradient of the convolution the fields above describe (h unused), as P partial sums per channel: x and gy
    // (mifft_conv_grad_args; with gates mifft_conv_grad_gated_args) -> (P D, n / 2 + 1) complex values, unscaled
    int64_t P = 0;
    bool grad = false;
    // word 10 of a filter-gradient payload: the stage of the fused partitioned filter gradient the plan is (0: none, the fused
    // gradient above).  1 / 2: the half spectra of the u-blocks / g-blocks of that geometry STORED, (batch, F, n / 2 + 1)
    // complex values, instead of summed (TileCfg::WSPEC); P slices the walk.  3: the lag-group correlation over such spectra
    // (lag_corr.hip): dims = {max(u_frames, 2), n}; U is (batch, u_frames, n / 2 + 1), stored frame j being frame u_first + j, G is
    // (batch, F, n / 2 + 1); out row (s, d, p), p < lag_groups, is the sum over slice s of the batch entries b of channel d,
    // ascending, and over f < F, ascending, of conj(U[b, d, f - p]) G[b, d, f] (mode bit 0: U[b, d, f + p], and the conjugate of
    // the sum is stored), frames outside the stored ones counting as zeros that are never read; P such slices.
    int stage = 0;
    int64_t lag_groups = 0, u_frames = 0, u_first = 0;
    uint32_t mode = 0;
    // bits 8..15 of the mode word: the STORAGE type of x, the gates and out (a filter-gradient plan: of x, gy and the gates), 0 the plan's
    // float type, or MIFFT_F16 / MIFFT_BF16 under an F32 plan: 2-byte elements widened in the load and rounded once in the
    // store (TileCfg::CONV).  in_dtype and out_dtype stay F32; elem_bytes is what a sample occupies in memory.
    int io = 0;
    // bit 0 the pregate (a tensor of x's shape that multiplies x as it is loaded), bit 1 the postgate (one of out's shape that
    // multiplies the result as it is stored); the tensors are arguments of every exec (mifft_gated_args), never plan state.
    // In a filter-gradient plan they are the forward plan's gates, fused into the loads of x and of gy
    uint32_t gates = 0;
    const void* h = nullptr;
    // the payload tagged MIFFT_CONV_PAIR_TAG (conv_pair_check): the second operand is a signal, v (batch, K, 1), one row per row
    // of x, and there is no filter spectrum (D = 1, h null).  Row r of x lies from index ea on in its n zero-extended samples,
    // row r of v from eb on; out[r] is the samples o .. o + Lo - 1 of irfft(rfft(xe) rfft(ve), n) (mode bit 0: the conjugate of
    // rfft(ve)).  x and v are arguments of every exec (mifft_conv_pair_args).  TileCfg::PAIR.
    bool pair = false;
    int64_t K = 0, ea = 0, eb = 0;
    bool is_conv() const { return D > 0; }  // (forward, gradient or pair)
    bool overlap_save() const { return S > 0; }
    bool partitioned() const { return Q > 0; }
    bool gated() const { return gates != 0; }
    bool gradient() const { return grad; }
    size_t elem_bytes(int float_dtype) const;
};

struct Plan {
    int device = 0;
    int in_dtype = MIFFT_F32, out_dtype = MIFFT_F32;
    int ndim = 1;
    int64_t dims[MIFFT_MAX_DIMS] = {};
    int64_t batch = 0;
    // mifft_plan_create_slab: the plan is one slab of a larger batch; every size-dependent choice (streaming twins, store
    // policy, cache policy, four-step threshold) is made for THIS many transforms, so that the slab's results equal the
    // same rows of one plan over the whole batch bit for bit.  0 = the plan's own batch.
    int64_t sel_batch = 0;
    double size_batch() const { return (double)(sel_batch > 0 ? sel_batch : batch); }
    int64_t prod = 1;
    // bytes one exec moves (the output-sized tensor read once and written once): what the size regimes of the kernel
    // families (streaming twins, non-temporal store windows) are measured in
    double exec_bytes() const { return size_batch() * (double)prod * (double)out_elem_bytes() * 2.0; }
    int in_components = 2;
    int inverse = 0;
    uint32_t flags = 0;
    int num_cus = 256;
    std::vector<DimPass> passes;  // in execution order: last dim first
    std::vector<std::vector<uint32_t>> stage_radices;  // per dim: the user's ordered stages (introspection)
    void* d_scratch = nullptr;  // four-step only: one tensor of the output size (the reference's calc_buf,
                                // fft/fft/_ndim_fft_gpu.mojo:185, exists for EVERY plan; here only for dims > 16384)
    size_t scratch_bytes = 0;
    bool alloc_failed = false;  // a route builder ran out of device memory: plan creation reports MIFFT_ERR_HIP
    // N-D transform whose `out` tensor fits the 256-MiB Infinity Cache: the first pass reads x with non-temporal loads
    // (x does not displace the row results) and later in-place passes alternate their walking direction
    bool cache_resident_nd = false;
    // plan creation only: the pass over dimension 1 has been given a half-store kernel (TileCfg::HS), which widens the cases
    // in which a Hermitian last pass pays (herm_pays)
    bool hs_selected = false;
    // plan creation only: the dimension the Hermitian last pass halves (index into dims).  1: the dimension of the pass right
    // before it, which then stores only half of its results; 2: the dimension the FIRST pass transforms -- the rows of a
    // three-pass 3-D plan, the column side of the plane of a 4-D one -- with a half-store first pass and a middle pass over the
    // lower half of its columns: every pass but the last then moves half the tensor.
    int herm_axis = 1;
    size_t in_elem_bytes() const;
    size_t out_elem_bytes() const;  // bytes of one complex output element
    // MIFFT_FLAG_HALF_SPECTRUM: the last dimension is stored as its n / 2 + 1 non-negative bins on the complex side
    // (out of a forward plan, x of an inverse one); prod_half = prod / n * (n / 2 + 1)
    bool half_spectrum() const { return (flags & MIFFT_FLAG_HALF_SPECTRUM) != 0; }
    // MIFFT_FLAG_KEEP_DIM: dims left untransformed (bit d = dim d)
    uint32_t keep_mask() const { return (flags & MIFFT_FLAG_KEEP_MASK) >> 8; }
    bool kept(int d) const { return ((keep_mask() >> d) & 1u) != 0; }
    int64_t prod_half = 0;
    // MIFFT_FLAG_DCT: both sides are (batch, n, 1) real tensors; what one exec moves is batch * n reals read and written
    bool dct() const { return (flags & MIFFT_FLAG_DCT) != 0; }
    // MIFFT_FLAG_DCT_ND: both sides are (batch, d0.., 1) real tensors (dctn.cpp); dct_any: either DCT flag
    bool dct_nd() const { return (flags & MIFFT_FLAG_DCT_ND) != 0; }
    bool dct_any() const { return dct() || dct_nd(); }
    double dct_exec_bytes() const { return size_batch() * (double)prod * (double)(out_elem_bytes() / 2) * 2.0; }
    // MIFFT_FLAG_STFT: dims = {T, n}; x is (batch, T, 1) real, out (batch, F, n / 2 + 1, 2), F = stft_frames() frames of n
    // samples every stft_hop(); stft_center(): 0 none, 1 reflect, 2 zeros (TileParams::stft_center)
    bool stft() const { return (flags & MIFFT_FLAG_STFT) != 0; }
    int64_t stft_hop() const { return (int64_t)((flags & MIFFT_FLAG_STFT_HOP_MASK) >> 16); }
    int stft_center() const { return (flags & MIFFT_FLAG_STFT_CENTER_REFLECT) ? 1 : (flags & MIFFT_FLAG_STFT_CENTER_ZEROS) ? 2 : 0; }
    int64_t stft_frames() const {
        if (istft_adj) return istft_adj;  // (the payload's: those of X, which `length` may have cropped)
        if (conv.is_conv()) return conv.F;  // (no frames, no hop: one row per batch entry, or the blocks of an overlap-save row)
        if (mdct) return (dims[0] + mdct - 1) / mdct + 1;
        return 1 + (stft_center() ? dims[0] : dims[0] - dims[1]) / stft_hop();
    }
    // the payload of such a plan tagged with MIFFT_MDCT_TAG: an MDCT of mdct = M = dims[1] / 2 coefficients per frame.
    // Frame f covers the samples [(f - 1) M, (f + 1) M) of its entry, F = ceil(T / M) + 1 frames; out is (batch, F, M, 1)
    // real, mdct_scale times the cosine sum over the windowed frame.  0: not one.  Set by mdct_detect.
    int64_t mdct = 0;
    double mdct_scale = 1.0;
    // a MIFFT_FLAG_ISTFT plan whose window payload is tagged with MIFFT_MDCT_TAG: the inverse MDCT of imdct = M = dims[2] / 2
    // coefficients per frame, dims = {T, F, 2 M}; x is (batch, F, M, 1) real, out (batch, T, 1).  0: not one.  Set by imdct_check.
    int64_t imdct = 0;
    // a MIFFT_FLAG_ISTFT plan whose window payload is tagged with MIFFT_STFT_ADJ_TAG: the adjoint of the STFT of signals of
    // dims[0] samples, dims = {T, F, n} -- 1: x is the incoming gradient (batch, F, n / 2 + 1, 2); 2 / 3: x is X itself and the
    // exec brings the real gradient of |X|^2 / |X| as `mult`, (batch, F, n / 2 + 1).  out is (batch, T, 1); with the reflect
    // bit the exec brings `edge`, (batch, 2, n / 2), too.  The centre bits mean what they mean on the forward.  0: not one.
    // Set by stft_adj_check.
    int stft_adj = 0;
    bool stft_adj_edges() const { return stft_adj && (flags & MIFFT_FLAG_STFT_CENTER_REFLECT) != 0; }
    // a MIFFT_FLAG_STFT plan whose window payload is tagged with MIFFT_ISTFT_ADJ_TAG: the adjoint of the inverse STFT plan of
    // istft_adj = F frames and dims[0] = T stored samples, dims = {T, n}; x is the incoming gradient (batch, T, 1), out
    // (batch, F, n / 2 + 1, 2).  MIFFT_FLAG_STFT_CENTER_ZEROS: the inverse plan is centred.  0: not one.  Set by istft_adj_check.
    int64_t istft_adj = 0;
    // a MIFFT_FLAG_STFT plan whose payload starts with MIFFT_CONV_TAG or MIFFT_CONV_GRAD_TAG: the decoded request (conv.cpp)
    ConvRequest conv;
    // a MIFFT_FLAG_DCT plan whose `bases` start with MIFFT_DCT_TYPE4_TAG: DCT-IV instead of DCT-II / DCT-III
    bool dct4 = false;
    // a MIFFT_FLAG_DCT / MIFFT_FLAG_DCT_ND plan whose `bases` start with MIFFT_DST_TAG (DST-II and its inverse, along every
    // transformed dim) or, MIFFT_FLAG_DCT only, with MIFFT_DST_TYPE4_TAG (DST-IV; dct4 is set as well): every pass is the
    // DCT plan's with DimPass::dst set
    bool dst = false;
    // MIFFT_FLAG_STFT_POWER on such a plan: out is real, (batch, F, n / 2 + 1, 1) of |X|^spec_power (1 or 2), or
    // (batch, F, spec_bands, 1) after a filterbank of spec_bands > 0 bands; stft_out_width() reals per frame.  0: the flag is
    // not set.  Filled by stft_unpack_bases.
    int spec_power = 0;
    int64_t spec_bands = 0;
    // The tagged payload (MIFFT_STFT_EXT_TAG) adds two stages to that store: spec_log -- y = fma(spec_a, log2(max(v +
    // spec_add, spec_amin)), spec_c), the four already rounded to the plan's float type -- and spec_post > 0, a dense
    // (spec_bands, spec_post) matrix applied to the bands of every frame; its weights follow the band weights in the band
    // table, spec_post_off elements behind their start (set by build_stft).
    bool spec_log = false;
    int64_t spec_post = 0;
    double spec_add = 0.0, spec_amin = 0.0, spec_a = 0.0, spec_c = 0.0;
    int64_t spec_post_off = 0;
    int64_t stft_out_width() const { return spec_post > 0 ? spec_post : spec_bands > 0 ? spec_bands : dims[1] / 2 + 1; }
    // MIFFT_FLAG_ISTFT: dims = {T, F, n}; x is (batch, F, n / 2 + 1, 2), out (batch, T, 1) real: F frames of n samples every
    // stft_hop() overlap-added over istft_padded_len() samples, of which T from istft_trim() on are stored
    bool istft() const { return (flags & MIFFT_FLAG_ISTFT) != 0; }
    bool istft_centered() const { return (flags & (MIFFT_FLAG_STFT_CENTER_REFLECT | MIFFT_FLAG_STFT_CENTER_ZEROS)) != 0; }
    int64_t istft_padded_len() const { return dims[2] + stft_hop() * (dims[1] - 1); }
    int64_t istft_trim() const { return istft_centered() ? dims[2] / 2 : 0; }
    // bytes of ONE transform (one batch entry) of x, out and the plan scratch: the slab offsets and the alias check of
    // mifft_exec_batch and the size queries.  Without the flag: prod * in_elem_bytes(), prod * out_elem_bytes() twice.
    size_t in_row_bytes() const;
    size_t out_row_bytes() const;
    size_t scratch_row_bytes() const;
};

// Hermitian twins: the trailing dimensions of the column space of the last pass (dims[1..ndim-1], at most three; absent
// leading ones are 1), and the flat prefix of columns that are not beyond their own mirror image
inline void herm_set_dims(const Plan& plan, DimPass& pass) {
    const int n = plan.ndim, a = plan.herm_axis;
    pass.herm_d2 = (int)plan.dims[n - 1];
    pass.herm_d1 = n >= 3 ? (int)plan.dims[n - 2] : 1;
    pass.herm_d0 = n >= 4 ? (int)plan.dims[n - 3] : 1;
    long long js = 1;
    for (int k = a + 1; k < n; ++k) js *= plan.dims[k];
    pass.herm_dj = (int)plan.dims[a];
    pass.herm_js = (int)js;
    pass.herm_L = (int)(plan.dims[a] * js);
    pass.herm_H = (int)((plan.dims[a] / 2 + 1) * js);
}
// tiles of `tile` columns that cover the transformed part of one image's column space
inline long long herm_tiles_per_outer(const DimPass& pass, int tile) {
    const long long rows = pass.inner / pass.herm_L, tpr = (pass.herm_H + tile - 1) / tile;
    return rows * tpr;
}

// Does a Hermitian twin (TileCfg::HERM) with `tile` columns per tile pay for this pass?  Measured with tools/herm_probe.py
// (DESIGN_EXPERIMENTS.md R3.6), whole transform against the ordinary kernels:
//   * tiles of whole 128-byte lines store their mirrored lines whole (contiguous runs with a carried column): 5-11 % at
//     every size when the rows of the trailing dimension are a whole number of tiles; ragged rows leave every mirrored line
//     in pieces (6 x 360^3 +3 %) unless the tensor stays in the Infinity Cache, where the pieces merge;
//   * narrower tiles (strided dimensions beyond ~1024 points) store every mirrored line in pieces: alone a gain (3-15 %) only
//     while the tensor is cache resident (with the table's own three-pass configurations: 4K frames 7-16 %);
//   * with a half-store pass in front (plan.hs_selected: that pass skips half its writes) the ragged and the 4- / 8-column cases
//     pay beyond the cache too: 40 x 1920 x 1080 0.98 -> 0.91, 6 x 360^3 1.03 -> 0.93, 300 x 600 x 500 1.02 -> 0.95;
//   * a Hermitian tile stores twice what an ordinary one does, so half the tiles must also mean clearly fewer ROUNDS of the
//     persistent grid: 1 x 64^4 (2112 tiles on 1024 workgroups: 3 rounds instead of 4) runs 12 % SLOWER, 1 x 256^3 (the
//     same 3 : 4, but four times the arithmetic per stored line) 5 % faster, 4 x 64^4 (9 : 16) 6 % faster.
inline bool herm_pays(const Plan& plan, const DimPass& pass, int tile, size_t lds_bytes, int threads) {
    if (config().herm == 2) return true;  // (lab build only: forced)
    const double out_bytes = plan.size_batch() * (double)plan.prod * (double)plan.out_elem_bytes();
    const bool resident = out_bytes <= (double)kInfinityCacheBytes;
    const long long d2 = plan.dims[plan.ndim - 1];
    const long long run_bytes = (long long)tile * (long long)plan.out_elem_bytes();
    if (run_bytes >= 128) {
        if (d2 % tile != 0 && !resident && !plan.hs_selected) return false;
    } else if (run_bytes < 32 || !(resident || plan.hs_selected)) {
        return false;
    }
    DimPass dims = pass;
    herm_set_dims(plan, dims);
    long long per_cu = (160 * 1024) / (long long)(lds_bytes ? lds_bytes : 1);  // the persistent grid, as tile_grid<>
    per_cu = std::max<long long>(1, std::min<long long>(std::min<long long>(per_cu, 2048 / (threads > 0 ? threads : 256)), 16));
    const long long grid = (long long)plan.num_cus * per_cu;
    const long long images = (long long)plan.size_batch() * pass.outer;
    const long long full = images * ((pass.inner + tile - 1) / tile);
    const long long half = images * herm_tiles_per_outer(dims, tile);
    const long long rounds_full = (full + grid - 1) / grid, rounds_half = (half + grid - 1) / grid;
    return (double)rounds_half <= (pass.N >= 128 ? 0.75 : 0.70) * (double)rounds_full;
}

// kernel families; each returns true and fills pass.launch/tile/... when it
// accepts the (plan, pass) pair.
bool select_generic(const Plan& plan, DimPass& pass, std::string& why_not);
bool select_fast(const Plan& plan, DimPass& pass);
// LAB BUILD ONLY (-DMIFFT_EXPERIMENTAL): wave-autonomous rows of N = 3 * R0 points: radix R0 in registers, radix 3 across
// three lanes by DPP (kernels_dpp.hip)
bool select_dpp_rows(const Plan& plan, DimPass& pass);
// the tile kernel specialised at plan time with hipRTC for a length without a table entry (kernels_jit.cpp)
bool select_jit(const Plan& plan, DimPass& pass, std::string& why_not);
// {tile, threads, n_tiles, grid} of the launch such a pass (or a precompiled packed-row one) makes for `count` batch entries,
// from the function the launch itself uses; false for a pass of another launcher (mifft_plan_pass_geometry)
bool tile_pass_geometry(const Plan& plan, const DimPass& pass, int64_t count, int64_t geometry_out[4]);
// interleaved block tile (TileCfg::ILV) of a masked plan's pass whose stride pass.inner holds fewer than 128 B of elements:
// false (+ the reason) when the length or the block does not fit it
bool select_jit_ilv(const Plan& plan, DimPass& pass, std::string& why_not);
// plans with a keep bit (MIFFT_FLAG_KEEP_DIM, axes.cpp): the checks that need no device, then the passes
int axes_check(const Plan& plan, std::string& why);
int build_axes(Plan& plan, const std::vector<std::vector<uint32_t>>& ordered,
               const std::vector<std::vector<uint32_t>>& processed, std::string& why);
// ---- the families of fused tile passes (kernels_jit.cpp) ------------------------------------------------------------------------
// Every fused feature is a variant of the packed-row (one: of the paired-column) tile kernel with a load or store of its own:
//   HalfRows   packed real rows of a half-spectrum plan: R2C (forward) or C2R (inverse) over the last dimension
//   DctRows    the same rows with TileCfg::DCT (DCT-II / its inverse; TileCfg::DST from the plan)
//   StftRows   R2C rows with TileCfg::STFT: the rows are the pass.outer frames of every batch entry (spectrogram stages and
//              TileCfg::IADJ from the plan)
//   ConvRows   R2C rows with TileCfg::CONV (overlap-save, partitions, gates, storage type, filter gradient, two signals: from plan.conv)
//   IstftRows  C2R rows with TileCfg::ISTFT: pass.outer frames per entry, overlap-added by the store (TileCfg::ADJ from the plan)
//   DctCols    the column tile with TileCfg::DCT: pass.N points at a stride of pass.inner PAIRS of real columns
//   Dct4Rows   complex rows of N / 2 points with TileCfg::DCT = 4 over rows of N reals
//   MdctRows   ... whose rows are the pass.outer lapped frames of every batch entry (TileCfg::MDCT)
//   ImdctRows  ... whose pass.outer frames per entry are unfolded and overlap-added by the store (TileCfg::IMDCT)
// Only HalfRows and DctRows have precompiled instances (below); the others are compiled at run time only.
// tile_family_supported: the family's check without a device, for the plan checks -- false + the reason
// (MIFFT_ERR_UNSUPPORTED) when the length (`inner`: the stride, DctCols only) has no configuration, or under MIFFT_JIT=0 no
// precompiled instance.  Pure.
// select_tile_family: the same check, then the kernel -- a precompiled instance or the runtime specialisation -- on the plan's
// device.  The pass must be FRESH: a newly constructed DimPass with dim_index, N, inner, outer, radices, processed, first and
// the buffer routing filled in (fused_row_pass below makes the usual one), as every caller's is.  On success launch, kernel_name,
// jit_fn, tile, threads and lds_bytes are the kernel's; every role field (r2c, c2r, dct, dst, mdct, imdct, stft, istft, conv,
// wgrad, hs, prefix_ok, ilv, herm_d0 .. 2) is cleared and then set from the configuration that was compiled, so the pass is
// what the kernel is; ld is the points the kernel runs (N / 2 of the row families, N of DctCols); IstftRows and ImdctRows
// carry Config::istft_min_run into istft_min_run, which enters the grid (tile_launch_geometry).  Scales and tables are the
// caller's.  On failure: false + the reason, the pass as it was.
enum class TileFamily { HalfRows, DctRows, StftRows, ConvRows, IstftRows, DctCols, Dct4Rows, MdctRows, ImdctRows };
bool tile_family_supported(TileFamily family, const Plan& plan, int64_t n, int64_t inner, std::string& why_not);
bool select_tile_family(TileFamily family, const Plan& plan, DimPass& pass, std::string& why_not);
// the precompiled packed-row kernels (kernels_half_rows.hip): the configuration's TileCfg type text, the kernel, its LDS bytes
struct HalfRowsKernel {
    const char* cfg;
    const void* fn;
    size_t lds_bytes;
};
const HalfRowsKernel* half_rows_kernels(int* count);
const HalfRowsKernel* dct_rows_kernels(int* count);  // (kernels_dct_rows.hip: the TileCfg::DCT instances)
// plans with MIFFT_FLAG_HALF_SPECTRUM (half_spectrum.cpp): the checks that need no device, then the passes (a status;
// plan.passes / d_scratch filled on success)
int half_spectrum_check(const Plan& plan, std::string& why);
int build_half_spectrum(Plan& plan, const std::vector<std::vector<uint32_t>>& ordered,
                        const std::vector<std::vector<uint32_t>>& processed, std::string& why);
// plans with MIFFT_FLAG_DCT (dct.cpp): the checks that need no device, then the single pass (DctRows, or Dct4Rows for a DCT-IV)
int dct_check(const Plan& plan, std::string& why);
hipError_t upload_dct4_table(int out_dtype, int64_t n, void** d_table);
int build_dct(Plan& plan, const std::vector<uint32_t>& ordered, const std::vector<uint32_t>& processed, std::string& why);
// ... its pieces, shared with the N-D plans: the packed-row pass over dimension dim_index (`outer` rows per batch entry), the
// scales of bin 0 and of the other bins, the table W_4n^k, k = 0 .. n / 2
int build_dct_rows(Plan& plan, int dim_index, int64_t outer, const std::vector<uint32_t>& ordered,
                   const std::vector<uint32_t>& processed, std::string& why);
void dct_scales(int64_t n, bool inverse, bool ortho, double& s0, double& s1);
hipError_t upload_quarter_table(int out_dtype, int64_t n, void** d_table);
// plans with MIFFT_FLAG_DCT_ND (dctn.cpp): the checks that need no device, then one pass per transformed dimension (DctRows
// over the last one, DctCols over the others)
int dctn_check(const Plan& plan, std::string& why);
int build_dctn(Plan& plan, const std::vector<std::vector<uint32_t>>& ordered,
               const std::vector<std::vector<uint32_t>>& processed, std::string& why);
// ---- the framed family: MIFFT_FLAG_STFT / MIFFT_FLAG_ISTFT plans and what their tagged payloads select -----------------------
// Which member a plan is: decided once, by framed_kind (mifft_api.cpp), from the mode bit and the *_detect predicates below.
enum class FramedKind { Stft, Istft, Adjoint, IstftAdjoint, Mdct, Imdct, Conv, ConvGrad, ConvPair };
// What a member's check decodes from `bases` for its build: the window (empty: rectangular), the filterbank and the matrix
// after the bands of a spectrogram plan, the gain of the inverse kinds, the user radices of the one transformed dim (empty:
// the default estimate).
struct FramedPayload {
    std::vector<double> window, fb, post;
    double gain = 1.0;
    std::vector<uint64_t> radices;
};
// a binary64 value as it travels through `bases`: two 32-bit words, low word first
inline double word_pair(const uint32_t* w) {
    const uint64_t bits = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
    double v;
    memcpy(&v, &bits, sizeof v);
    return v;
}
// the n window values at the front of a payload; a value that is not finite is MIFFT_ERR_BAD_BASES (stft.cpp)
int read_window(const uint32_t* bases_flat, int64_t n, std::vector<double>& window, std::string& why);
// the `count` user radices `off` words into bases_flat, behind the payload (stft.cpp)
void read_radices(const uint32_t* bases_flat, int64_t off, int count, std::vector<uint64_t>& radices);
// A kind's table of the flag bits it refuses, in the order it refuses them: the first one set in `flags` is
// MIFFT_ERR_UNSUPPORTED, "`prefix` + its text".
struct FlagRefusal {
    uint32_t bits;
    const char* what;
};
template <size_t N>
int refuse_flags(uint32_t flags, const FlagRefusal (&table)[N], const std::string& prefix, std::string& why) {
    for (const FlagRefusal& o : table)
        if (flags & o.bits) {
            why = prefix + o.what;
            return MIFFT_ERR_UNSUPPORTED;
        }
    return MIFFT_OK;
}
// plans with MIFFT_FLAG_STFT (stft.cpp): the checks that need no device (flags, shape, the window carried in `bases`), then
// the single pass (StftRows).  stft_flag_check: the STFT bits of a plan WITHOUT the flag.
int stft_flag_check(uint32_t flags, std::string& why);
int stft_check(const Plan& plan, std::string& why);
// the window of such a plan from bases_flat / bases_len (2 n words: the binary64 bits of w[0 .. n-1], low word first; none:
// rectangular, `window` left empty) and the user radices of the n-point transform (none: `radices` left empty).  With
// MIFFT_FLAG_STFT_POWER also the power and the filterbank (row-major (n / 2 + 1, M); M = 0: `fb` left empty), which set
// plan.spec_power and plan.spec_bands.  A payload with MIFFT_STFT_EXT_TAG in the power slot also carries the log stage and
// the (M, Q) matrix `post` (row-major; Q = 0: left empty), which set plan.spec_log, spec_add .. spec_c and plan.spec_post.
int stft_unpack_bases(Plan& plan, const uint32_t* bases_flat, const int32_t* bases_len, FramedPayload& payload, std::string& why);
int build_stft(Plan& plan, const std::vector<uint32_t>& ordered, const std::vector<uint32_t>& processed,
               const FramedPayload& payload, std::string& why);
// MDCT plans (the MIFFT_FLAG_STFT payload tagged with MIFFT_MDCT_TAG; stft.cpp).  mdct_detect: is bases_len[0] the tagged
// length 2 dims[1] + 4 with the tag behind the window?  (Pure; it looks at nothing else.)  mdct_check: everything that can be
// refused without a device, leaving the window, the scale (plan.mdct_scale) and the user radices of M / 2 in its outputs.
// build_mdct: the one pass, a DCT-IV tile with the framing, folding load.
bool mdct_detect(int ndim, const int64_t* dims, const uint32_t* bases_flat, const int32_t* bases_len);
int mdct_check(Plan& plan, const uint32_t* bases_flat, const int32_t* bases_len, FramedPayload& payload, std::string& why);
int build_mdct(Plan& plan, const std::vector<uint32_t>& ordered, const std::vector<uint32_t>& processed,
               const FramedPayload& payload, std::string& why);
// IMDCT plans (the MIFFT_FLAG_ISTFT payload tagged with MIFFT_MDCT_TAG; istft.cpp), in the same manner.  imdct_detect: does
// the window payload end in TAG | gain?  (Pure; the length itself is imdct_check's business.)  build_imdct: the one pass
// (ImdctRows).
bool imdct_detect(int ndim, const uint32_t* bases_flat, const int32_t* bases_len);
int imdct_check(Plan& plan, const uint32_t* bases_flat, const int32_t* bases_len, FramedPayload& payload, std::string& why);
int build_imdct(Plan& plan, const std::vector<uint32_t>& ordered, const std::vector<uint32_t>& processed,
                const FramedPayload& payload, std::string& why);
// Fused FFT convolution plans (the MIFFT_FLAG_STFT payload that starts with MIFFT_CONV_TAG; conv.cpp).  conv_detect: is
// bases_len[0] a tagged length (8, 12: overlap-save, 16: gated, or 20: partitioned) with the tag in front?  (Pure; it looks at nothing else.)  conv_check: everything that can
// be refused without a device, leaving the request in plan.conv and the user radices of n in `radices`.  build_conv: the
// one pass (ConvRows).  launch_jit_conv is its launch (kernels_jit.cpp), which -- unlike a DimPass::launch --
// knows the first row of the exec, for the filter row of every launch row, and takes the exec's two gates (null where the plan
// has none), offset to the exec's first signal row as `in` and `out` are.
bool conv_detect(int ndim, const uint32_t* bases_flat, const int32_t* bases_len);
int conv_check(Plan& plan, const uint32_t* bases_flat, const int32_t* bases_len, FramedPayload& payload, std::string& why);
int build_conv(Plan& plan, const std::vector<uint32_t>& ordered, const std::vector<uint32_t>& processed, std::string& why);
int launch_jit_conv(const Plan& plan, const DimPass& pass, const void* in, void* out, const void* pregate,
                    const void* postgate, int64_t first, int64_t count, hipStream_t stream);
// The filter-gradient plans (MIFFT_CONV_GRAD_TAG): the same trio and the launch of the whole batch; build_conv_grad picks P where the payload says 0
// for a built pass (pure arithmetic on its tile and the device's size).
bool conv_grad_detect(int ndim, const uint32_t* bases_flat, const int32_t* bases_len);
int conv_grad_check(Plan& plan, const uint32_t* bases_flat, const int32_t* bases_len, FramedPayload& payload, std::string& why);
int build_conv_grad(Plan& plan, const std::vector<uint32_t>& ordered, const std::vector<uint32_t>& processed, std::string& why);
int launch_jit_conv_grad(const Plan& plan, const DimPass& pass, const void* x, const void* gy, const void* pregate,
                         const void* postgate, void* out, hipStream_t stream);
// The two-signal plans (MIFFT_CONV_PAIR_TAG): the same trio; the pass is build_conv's with TileCfg::PAIR.  launch_jit_conv_pair
// is its launch, which takes the exec's two operands, offset to the exec's first row by the caller as `out` is.
bool conv_pair_detect(int ndim, const uint32_t* bases_flat, const int32_t* bases_len);
int conv_pair_check(Plan& plan, const uint32_t* bases_flat, const int32_t* bases_len, FramedPayload& payload, std::string& why);
int launch_jit_conv_pair(const Plan& plan, const DimPass& pass, const void* x, const void* v, void* out, int64_t count,
                         hipStream_t stream);
// workgroups per CU of a built tile-kernel pass's persistent grid (kernels_jit.cpp): the launches' rule, and build_conv_grad's
long long pass_wg_per_cu(const DimPass& pass);
// Stage 3 of the fused partitioned filter gradient (ConvRequest::stage; lag_corr.hip): the precompiled lag-group kernel.  A
// workgroup of kLagCorrThreads work items owns a channel, that many consecutive bins and a slice of the batch; the name is
// `lag_corr_<f32|f64>_p<bound>`, bound the compile-time count of accumulators (2, 4, 8, 16 or 32) that holds Pg.
// lag_corr_partials: P of a plan whose payload left it to the library -- 1 unless D times the bin groups alone leave the
// device short of workgroups, then enough slices of the batch to fill it, at most one per batch entry.
constexpr int kLagCorrThreads = 256;
const char* lag_corr_kernel_name(int dtype, int lag_groups);
int64_t lag_corr_partials(const Plan& plan);
int launch_lag_corr(const Plan& plan, const void* U, const void* G, void* out, hipStream_t stream);
// the band tables of such a plan, one device allocation (DimPass::d_aux3): lo[M], len[M], off[M] as int32, padded to an even
// count of ints, then the weights in the plan's float type, then the M Q weights of `post` in the same type
inline int64_t spec_table_ints(int64_t M) { return (3 * M + 1) / 2 * 2; }
// plans with MIFFT_FLAG_ISTFT (istft.cpp), in the same manner: istft_check needs no device and leaves the window (empty:
// rectangular), the gain and the user radices in its outputs; it refuses a window whose squared overlap-add is zero
// somewhere in the samples the plan stores.  build_istft: the one pass (IstftRows).
int istft_check(const Plan& plan, const uint32_t* bases_flat, const int32_t* bases_len, FramedPayload& payload, std::string& why);
int build_istft(Plan& plan, const std::vector<uint32_t>& ordered, const std::vector<uint32_t>& processed,
                const FramedPayload& payload, std::string& why);
// STFT adjoint plans (the MIFFT_FLAG_ISTFT payload tagged with MIFFT_STFT_ADJ_TAG; istft.cpp).  stft_adj_detect: is
// bases_len[0] the tagged length 2 n + 6 with the tag behind the window?  (Pure.)  stft_adj_check: istft_check's refusals
// less the ones an adjoint has no use for (the covered length, the overlap-add condition), each reason naming the adjoint;
// sets plan.stft_adj.  build_istft builds the pass (no envelope table).  launch_stft_adj is its launch, which takes the
// exec's factor and edge tensors (null where the plan has none), offset to the exec's first entry as `in` and `out` are.
bool stft_adj_detect(int ndim, const int64_t* dims, const uint32_t* bases_flat, const int32_t* bases_len);
int stft_adj_check(Plan& plan, const uint32_t* bases_flat, const int32_t* bases_len, FramedPayload& payload, std::string& why);
int launch_stft_adj(const Plan& plan, const DimPass& pass, const void* in, const void* mult, void* out, void* edge,
                    int64_t count, hipStream_t stream);
// Inverse STFT adjoint plans (the MIFFT_FLAG_STFT payload tagged with MIFFT_ISTFT_ADJ_TAG; istft.cpp, beside the envelope
// they share with the inverse plan).  istft_adj_detect: is bases_len[0] the tagged length 2 n + 6 with the tag behind the
// window?  (Pure.)  istft_adj_check: the limits of the inverse plan it is the adjoint of (hop, covered length, the 2^26
// padded samples, the overlap-add condition), then the STFT tile's; sets plan.istft_adj, the payload's frame count.
// build_istft_adj: the STFT pass with TileCfg::IADJ over that many frames per entry, the reciprocal envelope in d_aux3.
bool istft_adj_detect(int ndim, const int64_t* dims, const uint32_t* bases_flat, const int32_t* bases_len);
int istft_adj_check(Plan& plan, const uint32_t* bases_flat, const int32_t* bases_len, FramedPayload& payload, std::string& why);
int build_istft_adj(Plan& plan, const std::vector<uint32_t>& ordered, const std::vector<uint32_t>& processed,
                    const FramedPayload& payload, std::string& why);
// first pass over a REAL tensor whose last pass will be a Hermitian twin: rows read as N / 2 packed complex points, unpacked
// into the half spectrum by the store loop (TileCfg::R2C); pass.want_half asks for it.  LAB BUILD ONLY.
bool select_jit_r2c(const Plan& plan, DimPass& pass, std::string& why_not);
// four-step helpers: the transposed + twiddled column pass (reads x: real / integer input allowed) and cheap
// feasibility predicates for scoring factorisations without compiling
bool select_jit_streaming_rows(const Plan& plan, DimPass& pass, std::string& why_not);  // LAB BUILD ONLY
// the non-temporal-store window of batched 1-D transforms (bytes moved per exec, kernels_fast.hip; Config::nts_*)
bool nts_window(const Plan& plan, double total_bytes);
// contiguous dimension of N1 * N2 points as a four-step inside one LDS plane (kernels_fast.hip)
bool select_row2d(const Plan& plan, DimPass& pass);
bool nts_window_bytes(double total_bytes);  // the same window without the one-dimension condition (single-pass planes)
bool select_jit_plane(const Plan& plan, DimPass& pass, std::string& why_not);
// LAB BUILD ONLY: the two innermost dimensions of images that fit one XCD's L2: rows, XCD-local barrier, columns from L2
bool select_jit_image(const Plan& plan, DimPass& pass, std::string& why_not);
bool select_jit_tstore(const Plan& plan, DimPass& pass, std::string& why_not);
// first four-step pass of a strided dimension (TileCfg::FS1): pass.N = N1, pass.fs_n2 = N2
bool select_jit_fs1(const Plan& plan, DimPass& pass, std::string& why_not);
// a strided dimension beyond one column tile as two column passes through the plan scratch (kernels_fourstep.hip)
bool build_fourstep_strided(Plan& plan, int dim_index, std::string& why_not);
bool jit_tstore_feasible(const Plan& plan, int64_t n1, int64_t n2);
bool jit_cols_feasible(const Plan& plan, int64_t n, int64_t inner);
int jit_precompile(int in_dtype, int out_dtype, int64_t n, int cols, int in_real, size_t* code_bytes, std::string& why);
// fused pass over the two innermost dimensions (pass.N = contiguous dim, pass.N1 = the next one)
bool select_fast_plane(const Plan& plan, DimPass& pass);
// a contiguous dimension too long for one workgroup: three passes (column FFTs of N1, transpose + twiddle,
// column FFTs of N2).  Appends its passes to plan.passes and allocates plan.d_scratch.
bool build_fourstep(Plan& plan, int dim_index, std::string& why_not);
// a strided dimension too long for an in-place column tile: transpose -> row kernel -> transpose through the scratch
bool build_transposed_dim(Plan& plan, int dim_index, const std::vector<uint32_t>& radices,
                          const std::vector<uint32_t>& processed, std::string& why_not);
hipError_t upload_twiddle_table(int out_dtype, int64_t N, bool inverse, void** d_table);
// ---- what the builders of the fused passes share --------------------------------------------------------------------------------
// The fresh DimPass of a single fused row pass over dimension dim_index: n points, `outer` rows (frames, blocks) per batch
// entry, reading x.  half_pitch: the complex side has rows of n / 2 + 1 bins.
inline DimPass fused_row_pass(int dim_index, int64_t n, int64_t outer, const std::vector<uint32_t>& radices,
                              const std::vector<uint32_t>& processed, bool half_pitch) {
    DimPass ps;
    ps.dim_index = dim_index;
    ps.N = n;
    ps.outer = outer;
    ps.radices = radices;
    ps.processed = processed;
    ps.first = true;
    if (half_pitch) ps.half_pitch = n / 2 + 1;
    return ps;
}
// the table pair of a packed-row pass (r2c / c2r): the passes run N / 2 points, d_twiddle is that table in the given direction;
// the fold / unpacking needs W_N^k, forward, in d_aux
inline hipError_t upload_packed_tables(int out_dtype, bool inverse, DimPass& ps) {
    hipError_t e = upload_twiddle_table(out_dtype, ps.N / 2, inverse, &ps.d_twiddle);
    if (e == hipSuccess) e = upload_twiddle_table(out_dtype, ps.N, false, &ps.d_aux);
    return e;
}
// the end of every builder: the pass joins the plan BEFORE the status of its uploads is looked at (the plan's owner frees what
// has been uploaded), then that status, under the name `what`
inline int append_pass(Plan& plan, const DimPass& ps, hipError_t e, const char* what) {
    plan.passes.push_back(ps);
    return e == hipSuccess ? MIFFT_OK : hip_error(e, what);
}
// every other plan (schedule.cpp): the general route, one kernel per pass over every dimension chosen by its scheduler
int build_general(Plan& plan, const std::vector<std::vector<uint32_t>>& ordered,
                  const std::vector<std::vector<uint32_t>>& processed, std::string& why);
// Frees the device tables of every pass and the plan scratch (schedule.cpp).  No HIP call for a plan that owns nothing: it
// also runs where no device was opened.
void free_plan_device(Plan& plan);

inline size_t dtype_size(int dt) {
    switch (dt) {
        case MIFFT_F32: return 4;
        case MIFFT_F64: return 8;
        case MIFFT_U8: return 1;
        case MIFFT_I32: return 4;
        case MIFFT_I8: return 1;
        case MIFFT_I16: return 2;
        case MIFFT_U16: return 2;
        case MIFFT_F16: return 2;
        case MIFFT_BF16: return 2;
    }
    return 0;
}
inline size_t ConvRequest::elem_bytes(int float_dtype) const { return io ? 2 : dtype_size(float_dtype); }

}  // namespace mifft

// the opaque C handle
struct mifft_plan {
    mifft::Plan p;
};
