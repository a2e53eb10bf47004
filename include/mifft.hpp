// mifft.hpp -- C++ host mirror of the reference's GPU call surface, header-only, on top of the C ABI (mifft.h).
//
// The reference is compiled code (Mojo); where its toolchain is absent the host side above the C ABI is C++ with the
// reference's names, argument meaning and error behaviour:
//
//   reference (fft/fft/fft.mojo)                                              here
//   plan_fft[in_dtype, out_dtype, in_layout, out_layout, *, bases, inverse]   mifftxx::plan_fft(in_dtype, out_dtype, in_layout,
//       (ctx: DeviceContext) raises -> _GPUPlan          (:161-210)               out_layout, ctx, bases, inverse) -> mifftxx::Plan
//   fft(output, x, ctx, *, plan) raises                  (:262-323)           mifftxx::fft(output, x, ctx, plan)
//   _estimate_best_bases[length, target]()               (:49-104)            mifftxx::estimate_best_bases(length, "gpu" | "cpu")
//   _get_ordered_bases_processed_list (fft/fft/_utils.mojo:186-221)           mifftxx::ordered_bases(length, bases)
//
// (Namespace mifftxx: `mifft` is the library's internal namespace.)
// Layouts are row-major (batches, d0[, d1 ...], C) with C_out = 2 and C_in in {1, 2} (fft/fft/fft.mojo:20-46); what the
// reference rejects with compile-time asserts (:22-46, _utils.mojo:189-220) throws mifftxx::Error with the reference's
// message BEFORE any device work.  `output` / `x` are device pointers on ctx.device; `fft` enqueues on ctx.stream and
// returns (the caller synchronises, fft/bench.mojo:51-52).  Link with -lmifft; nothing else is needed (no HIP headers).
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "mifft.h"

namespace mifftxx {

struct Error : std::runtime_error {
    int status;
    Error(int s, const std::string& m) : std::runtime_error("mifft error " + std::to_string(s) + ": " + m), status(s) {}
};

// DeviceContext of the reference: a device and the stream its work is enqueued on (NULL = the default stream)
struct DeviceContext {
    int device = 0;
    void* stream = nullptr;  // hipStream_t
};

inline void check(int rc) {
    if (rc < 0) throw Error(rc, mifft_last_error());
}

inline std::vector<uint32_t> ordered_bases(uint32_t length, const std::vector<uint32_t>& bases) {
    std::vector<uint32_t> out(MIFFT_MAX_STAGES);
    const int n = mifft_ordered_bases(length, bases.data(), (int)bases.size(), out.data(), (int)out.size());
    check(n);
    out.resize(n);
    return out;
}

inline std::vector<uint32_t> estimate_best_bases(uint32_t length, const std::string& target = "gpu") {
    std::vector<uint32_t> out(MIFFT_MAX_STAGES);
    const int n = mifft_estimate_bases(length, target == "gpu" ? 1 : 0, out.data(), (int)out.size());
    check(n);
    out.resize(n);
    return out;
}

// _GPUPlan (fft/fft/_ndim_fft_gpu.mojo:153-207): owns the device twiddle tables (and a scratch tensor on three routes only)
class Plan {
   public:
    Plan() = default;
    Plan(const Plan&) = delete;
    Plan& operator=(const Plan&) = delete;
    Plan(Plan&& o) noexcept { *this = std::move(o); }
    Plan& operator=(Plan&& o) noexcept {
        if (this != &o) {
            reset();
            h_ = o.h_;
            in_layout = std::move(o.in_layout);
            out_layout = std::move(o.out_layout);
            o.h_ = nullptr;
        }
        return *this;
    }
    ~Plan() { reset(); }

    std::vector<uint32_t> stages(int dim) const {
        std::vector<uint32_t> out(MIFFT_MAX_STAGES);
        const int n = mifft_plan_stages(h_, dim, out.data(), (int)out.size());
        check(n);
        out.resize(n);
        return out;
    }
    std::string kernel_name(int dim) const { return mifft_plan_kernel_name(h_, dim); }
    int num_launches() const { return mifft_plan_num_launches(h_); }
    // {tile, threads, n_tiles, grid} of the launch for dimension `dim` over `count` batch entries
    std::vector<int64_t> pass_geometry(int dim, int64_t count) const {
        std::vector<int64_t> g(4);
        check(mifft_plan_pass_geometry(h_, dim, count, g.data()));
        return g;
    }
    size_t in_bytes() const { return mifft_plan_in_bytes(h_); }
    size_t out_bytes() const { return mifft_plan_out_bytes(h_); }
    size_t scratch_bytes() const { return mifft_plan_scratch_bytes(h_); }
    const mifft_plan* handle() const { return h_; }

    std::vector<int64_t> in_layout, out_layout;

   private:
    friend Plan plan_fft(mifft_dtype, mifft_dtype, const std::vector<int64_t>&, const std::vector<int64_t>&,
                         const DeviceContext&, const std::vector<std::vector<uint32_t>>*, bool, uint32_t);
    void reset() {
        if (h_) mifft_plan_destroy(h_);
        h_ = nullptr;
    }
    mifft_plan* h_ = nullptr;
};

// _check_layout_conditions_nd (fft/fft/fft.mojo:20-46), with the reference's assert texts
inline void check_layout_conditions_nd(const std::vector<int64_t>& in_layout, const std::vector<int64_t>& out_layout) {
    const size_t rank = out_layout.size();
    if (rank <= 2) throw Error(MIFFT_ERR_BAD_RANK, "The rank should be bigger than 2.");
    if (in_layout.size() != rank) throw Error(MIFFT_ERR_BAD_RANK, "in_layout and out_layout must have equal rank");
    if (in_layout[rank - 1] != 1 && in_layout[rank - 1] != 2)
        throw Error(MIFFT_ERR_BAD_COMPONENTS, "The last dimension of in_layout should be 1 or 2");
    if (out_layout[rank - 1] != 2) throw Error(MIFFT_ERR_BAD_COMPONENTS, "out_layout must have the last dimension equal to 2");
    for (size_t i = 0; i + 1 < rank; ++i)
        if (in_layout[i] != out_layout[i])
            throw Error(MIFFT_ERR_BAD_DIM, "out_layout and in_layout should have the same shape before the last dimension");
    for (size_t i = 1; i + 1 < rank; ++i)
        if (out_layout[i] == 1) throw Error(MIFFT_ERR_BAD_DIM, "no inner dimension should be of size 1");
}

// plan_fft, GPU overload (fft/fft/fft.mojo:161-210).  bases == nullptr: the reference's default
// (_estimate_best_bases_nd[.., "gpu"]).  `runtime_twfs` / `max_cluster_size` have no MI355X meaning; `_test` maps to
// flags = MIFFT_FLAG_FAITHFUL_STAGES (the user's stages run literally, one LDS pass each).  With MIFFT_FLAG_HALF_SPECTRUM the
// layouts are those of include/mifft.h: the last dimension of the complex side holds h = n / 2 + 1 bins (checked by the
// library: mifft_plan_create receives the logical real dims).  MIFFT_FLAG_KEEP_DIM(d) leaves dim d untransformed (its bases
// list, when given, is empty).  MIFFT_FLAG_DCT (with MIFFT_FLAG_DCT_ORTHO for norm = "ortho") plans a DCT-II, or with
// `inverse` its inverse, of real rows: its layouts are (batch, n, 1) on BOTH sides, which check_layout_conditions_nd refuses
// (it wants a complex out_layout), so such a plan is created through mifft_plan_create itself.  The same holds for
// MIFFT_FLAG_DCT_ND (16u), the N-D DCT over real (batch, d0.., 1) tensors, keep bits allowed.
static_assert(MIFFT_FLAG_DCT_ND == 16u && (MIFFT_FLAG_DCT_ND & (MIFFT_FLAG_DCT | MIFFT_FLAG_DCT_ORTHO | MIFFT_FLAG_KEEP_MASK)) == 0,
              "MIFFT_FLAG_DCT_ND is its own bit");
// MIFFT_FLAG_STFT (32u) with MIFFT_FLAG_STFT_HOP(hop) and at most one of MIFFT_FLAG_STFT_CENTER_REFLECT (64u) /
// MIFFT_FLAG_STFT_CENTER_ZEROS (128u) plans the short-time Fourier transform of real signals: x (batch, T, 1) ->
// out (batch, F, n / 2 + 1, 2), dims = {T, n}.  The two layouts differ before the last dimension and `bases` carries the window
// (include/mifft.h), so such a plan, too, is created through mifft_plan_create itself.
static_assert(MIFFT_FLAG_STFT == 32u && MIFFT_FLAG_STFT_CENTER_REFLECT == 64u && MIFFT_FLAG_STFT_CENTER_ZEROS == 128u &&
                  MIFFT_FLAG_STFT_HOP(1) == 0x10000u && MIFFT_FLAG_STFT_HOP_MASK == 0xFFFF0000u &&
                  ((MIFFT_FLAG_STFT | MIFFT_FLAG_STFT_CENTER_REFLECT | MIFFT_FLAG_STFT_CENTER_ZEROS | MIFFT_FLAG_STFT_HOP_MASK) &
                   (MIFFT_FLAG_KEEP_MASK | MIFFT_FLAG_DCT_ND | MIFFT_FLAG_DCT | MIFFT_FLAG_DCT_ORTHO | MIFFT_FLAG_HALF_SPECTRUM |
                    MIFFT_FLAG_FAITHFUL_STAGES)) == 0,
              "the STFT bits are their own");
// MIFFT_FLAG_ISTFT (0x4000u) with MIFFT_FLAG_STFT_HOP(hop) and at most one centre bit plans the inverse, real output:
// x (batch, F, n / 2 + 1, 2) -> out (batch, T, 1), dims = {T, F, n}; `bases` carries the window and a gain (include/mifft.h).
// Created through mifft_plan_create itself, as the forward.
static_assert(MIFFT_FLAG_ISTFT == 0x4000u &&
                  (MIFFT_FLAG_ISTFT & (MIFFT_FLAG_STFT | MIFFT_FLAG_STFT_CENTER_REFLECT | MIFFT_FLAG_STFT_CENTER_ZEROS |
                                       MIFFT_FLAG_STFT_HOP_MASK | MIFFT_FLAG_KEEP_MASK | MIFFT_FLAG_DCT_ND | MIFFT_FLAG_DCT |
                                       MIFFT_FLAG_DCT_ORTHO | MIFFT_FLAG_HALF_SPECTRUM | MIFFT_FLAG_FAITHFUL_STAGES)) == 0,
              "MIFFT_FLAG_ISTFT is its own bit");
// MIFFT_FLAG_STFT_POWER (0x8000u) beside MIFFT_FLAG_STFT: the same plan with a REAL output, |X|^power (1 or 2) as
// (batch, F, n / 2 + 1, 1), or its product with an (n / 2 + 1, M) filterbank as (batch, F, M, 1); `bases` carries the window,
// the power and the filterbank (include/mifft.h).  Created through mifft_plan_create itself, as the STFT plan.
static_assert(MIFFT_FLAG_STFT_POWER == 0x8000u &&
                  (MIFFT_FLAG_STFT_POWER & (MIFFT_FLAG_ISTFT | MIFFT_FLAG_STFT | MIFFT_FLAG_STFT_CENTER_REFLECT |
                                            MIFFT_FLAG_STFT_CENTER_ZEROS | MIFFT_FLAG_STFT_HOP_MASK | MIFFT_FLAG_KEEP_MASK |
                                            MIFFT_FLAG_DCT_ND | MIFFT_FLAG_DCT | MIFFT_FLAG_DCT_ORTHO | MIFFT_FLAG_HALF_SPECTRUM |
                                            MIFFT_FLAG_FAITHFUL_STAGES)) == 0,
              "MIFFT_FLAG_STFT_POWER is its own bit");
// The tag of the extended payload of such a plan (log stage, matrix after the bands): a quiet NaN in the power slot.
static_assert(MIFFT_STFT_EXT_TAG_LO == 0x46465401u && MIFFT_STFT_EXT_TAG_HI == 0x7FF84D49u &&
                  (MIFFT_STFT_EXT_TAG_HI & 0x7FF80000u) == 0x7FF80000u,
              "MIFFT_STFT_EXT_TAG is the quiet NaN 0x7FF84D4946465401");
constexpr uint64_t kStftExtTag = ((uint64_t)MIFFT_STFT_EXT_TAG_HI << 32) | MIFFT_STFT_EXT_TAG_LO;
// MIFFT_DCT_TYPE4_TAG as the first `bases` word of a MIFFT_FLAG_DCT plan: DCT-IV of real rows (no radix can equal the tag).
// MIFFT_MDCT_TAG behind the 2 M window values of a MIFFT_FLAG_STFT | MIFFT_FLAG_STFT_CENTER_ZEROS | MIFFT_FLAG_STFT_HOP(M)
// plan with dims = {T, 2 M}: the MDCT, x (batch, T, 1) -> out (batch, F, M, 1) real (include/mifft.h).  The same tag behind
// the window of a MIFFT_FLAG_ISTFT | MIFFT_FLAG_STFT_CENTER_ZEROS | MIFFT_FLAG_STFT_HOP(M) plan with dims = {T, F, 2 M} and
// inverse = 1: the IMDCT, x (batch, F, M, 1) -> out (batch, T, 1).  All are created through mifft_plan_create itself, as the
// plans above.
static_assert(MIFFT_DCT_TYPE4_TAG == 0x44435434u && MIFFT_DCT_TYPE4_TAG > 16384u, "MIFFT_DCT_TYPE4_TAG is no radix");
static_assert(MIFFT_MDCT_TAG_LO == 0x43544401u && MIFFT_MDCT_TAG_HI == 0x7FF84D44u &&
                  (MIFFT_MDCT_TAG_HI & 0x7FF80000u) == 0x7FF80000u &&
                  (MIFFT_MDCT_TAG_HI != MIFFT_STFT_EXT_TAG_HI || MIFFT_MDCT_TAG_LO != MIFFT_STFT_EXT_TAG_LO),
              "MIFFT_MDCT_TAG is the quiet NaN 0x7FF84D4443544401, distinct from MIFFT_STFT_EXT_TAG");
// MIFFT_DST_TAG in the same place on a MIFFT_FLAG_DCT or MIFFT_FLAG_DCT_ND plan: DST-II (inverse: its inverse) of real rows, or
// along every transformed dim; MIFFT_DST_TYPE4_TAG on a MIFFT_FLAG_DCT plan: DST-IV of real rows (include/mifft.h).
static_assert(MIFFT_DST_TAG == 0x44535432u && MIFFT_DST_TYPE4_TAG == 0x44535434u && MIFFT_DST_TAG > 16384u,
              "MIFFT_DST_TAG and MIFFT_DST_TYPE4_TAG are no radices");
constexpr uint32_t kDctType4Tag = MIFFT_DCT_TYPE4_TAG;
constexpr uint32_t kDstTag = MIFFT_DST_TAG;
constexpr uint32_t kDstType4Tag = MIFFT_DST_TYPE4_TAG;
constexpr uint64_t kMdctTag = ((uint64_t)MIFFT_MDCT_TAG_HI << 32) | MIFFT_MDCT_TAG_LO;
// (In front of 12 words -- TAG | D | c | S | mode | H | F | s0 | Lo | 0 -- it is the overlap-save form for rows of any length T:
// F blocks of n samples every S per row, of which the S samples from c on are stored; that c and S keep the stored samples free
// of wrap-around, c >= K - 1 and c + S <= n for K taps, is the caller's contract.  mifft.h has the table.)
// MIFFT_CONV_TAG as the FIRST two words of the 8-word payload of a plain MIFFT_FLAG_STFT plan with dims = {L, n}: the fused FFT
// convolution of real rows, x (batch, L, 1) -> out (batch, Lo, 1), against the caller's device buffer of filter spectra
// (TAG | D | o | Lo | mode | address; include/mifft.h).  Created through mifft_plan_create itself.
static_assert(MIFFT_CONV_TAG_LO == 0x4F4E5601u && MIFFT_CONV_TAG_HI == 0x7FF84D43u &&
                  (MIFFT_CONV_TAG_HI & 0x7FF80000u) == 0x7FF80000u && MIFFT_CONV_TAG_HI != MIFFT_MDCT_TAG_HI &&
                  MIFFT_CONV_TAG_HI != MIFFT_STFT_EXT_TAG_HI,
              "MIFFT_CONV_TAG is the quiet NaN 0x7FF84D434F4E5601, distinct from the other payload tags");
constexpr uint64_t kConvTag = ((uint64_t)MIFFT_CONV_TAG_HI << 32) | MIFFT_CONV_TAG_LO;
// (In front of 16 words -- the eight | F (0: single block) | s0 | Lo | gates | 0 0 0 0 -- either form with an elementwise pregate
// (bit 0, x's shape) and postgate (bit 1, out's shape) fused into the tile's load and store.  The gates are arguments of every
// exec: mifft_exec_batch takes the host address of a mifft_gated_args {MIFFT_GATED_ARGS_MAGIC, x, pregate, postgate} as its x.)
static_assert(MIFFT_GATED_ARGS_MAGIC == 0x314147544646494Dull && sizeof(mifft_gated_args) == 8 + 3 * sizeof(void*),
              "mifft_gated_args is the magic word \"MIFFTGA1\" and three pointers");
// MIFFT_CONV_GRAD_TAG in front of 16 words -- TAG | D | c | S | mode | F | s0 | Lo | P | 0 x 6 -- on the same kind of plan: the
// filter gradient of such a convolution, x (batch, L, 1) and gy (batch, Lo, 1) -> out (P D, n / 2 + 1, 2), unscaled partial
// sums of conj(U) G per channel.  The exec takes the host address of a mifft_conv_grad_args {MIFFT_CONV_GRAD_ARGS_MAGIC, x, gy}
// as its x and covers the whole batch (include/mifft.h).  Word 11 of the payload: the forward plan's gates (0 none, bit 0 the
// pregate, bit 1 the postgate), multiplied into the loads of x and gy; such a plan's exec takes a mifft_conv_grad_gated_args
// {MIFFT_CONV_GRAD_GATED_ARGS_MAGIC, x, gy, pregate, postgate}.
static_assert(MIFFT_CONV_GRAD_TAG_LO == 0x44524701u && MIFFT_CONV_GRAD_TAG_HI == 0x7FF84D47u &&
                  (MIFFT_CONV_GRAD_TAG_HI & 0x7FF80000u) == 0x7FF80000u && MIFFT_CONV_GRAD_TAG_HI != MIFFT_CONV_TAG_HI &&
                  MIFFT_CONV_GRAD_TAG_HI != MIFFT_MDCT_TAG_HI && MIFFT_CONV_GRAD_TAG_HI != MIFFT_STFT_EXT_TAG_HI,
              "MIFFT_CONV_GRAD_TAG is the quiet NaN 0x7FF84D4744524701, distinct from the other payload tags");
constexpr uint64_t kConvGradTag = ((uint64_t)MIFFT_CONV_GRAD_TAG_HI << 32) | MIFFT_CONV_GRAD_TAG_LO;
static_assert(MIFFT_CONV_GRAD_ARGS_MAGIC == 0x314757544646494Dull && sizeof(mifft_conv_grad_args) == 8 + 2 * sizeof(void*),
              "mifft_conv_grad_args is the magic word \"MIFFTWG1\" and two pointers");
static_assert(MIFFT_CONV_GRAD_GATED_ARGS_MAGIC == 0x324757544646494Dull && sizeof(mifft_conv_grad_gated_args) == 8 + 4 * sizeof(void*),
              "mifft_conv_grad_gated_args is the magic word \"MIFFTWG2\" and four pointers");
// MIFFT_CONV_PAIR_TAG in front of 16 words -- TAG | K | ea | eb | o | Lo | mode | 0 x 8 -- on the same kind of plan: the
// convolution (mode bit 0: correlation) of two signal batches row by row, x (batch, L, 1) and v (batch, K, 1) -> out
// (batch, Lo, 1), with no filter spectrum.  The exec takes the host address of a mifft_conv_pair_args
// {MIFFT_CONV_PAIR_ARGS_MAGIC, x, v} as its x (include/mifft.h).
static_assert(MIFFT_CONV_PAIR_TAG_LO == 0x49415001u && MIFFT_CONV_PAIR_TAG_HI == 0x7FF84D50u &&
                  (MIFFT_CONV_PAIR_TAG_HI & 0x7FF80000u) == 0x7FF80000u && MIFFT_CONV_PAIR_TAG_HI != MIFFT_CONV_TAG_HI &&
                  MIFFT_CONV_PAIR_TAG_HI != MIFFT_CONV_GRAD_TAG_HI && MIFFT_CONV_PAIR_TAG_HI != MIFFT_MDCT_TAG_HI &&
                  MIFFT_CONV_PAIR_TAG_HI != MIFFT_STFT_EXT_TAG_HI && MIFFT_CONV_PAIR_TAG_HI != MIFFT_STFT_ADJ_TAG_HI &&
                  MIFFT_CONV_PAIR_TAG_HI != MIFFT_ISTFT_ADJ_TAG_HI,
              "MIFFT_CONV_PAIR_TAG is the quiet NaN 0x7FF84D5049415001, distinct from the other payload tags");
constexpr uint64_t kConvPairTag = ((uint64_t)MIFFT_CONV_PAIR_TAG_HI << 32) | MIFFT_CONV_PAIR_TAG_LO;
static_assert(MIFFT_CONV_PAIR_ARGS_MAGIC == 0x314150544646494Dull && sizeof(mifft_conv_pair_args) == 8 + 2 * sizeof(void*),
              "mifft_conv_pair_args is the magic word \"MIFFTPA1\" and two pointers");
inline Plan plan_fft(mifft_dtype in_dtype, mifft_dtype out_dtype, const std::vector<int64_t>& in_layout,
                     const std::vector<int64_t>& out_layout, const DeviceContext& ctx,
                     const std::vector<std::vector<uint32_t>>* bases = nullptr, bool inverse = false,
                     uint32_t flags = MIFFT_FLAG_NONE) {
    check_layout_conditions_nd(in_layout, out_layout);
    const int ndim = (int)out_layout.size() - 2;
    if (bases && (int)bases->size() != ndim)
        throw Error(MIFFT_ERR_NO_BASES, "The bases list should have the same outer size as the amount of internal dimensions. "
                                        "e.g. (batches, dim_0, dim_1, dim_2, 2) -> len(bases) == 3");
    std::vector<uint32_t> flat;
    std::vector<int32_t> lens;
    if (bases)
        for (const auto& b : *bases) {
            lens.push_back((int32_t)b.size());
            flat.insert(flat.end(), b.begin(), b.end());
        }
    Plan p;
    p.in_layout = in_layout;
    p.out_layout = out_layout;
    check(mifft_plan_create(&p.h_, ctx.device, in_dtype, out_dtype, ndim, out_layout.data() + 1, out_layout[0],
                            (int)in_layout.back(), inverse ? 1 : 0, bases ? flat.data() : nullptr,
                            bases ? lens.data() : nullptr, flags));
    return p;
}

// fft, GPU overload (fft/fft/fft.mojo:262-323): out of place, x never written, every element of output written;
// asynchronous on ctx.stream
inline void fft(void* output, const void* x, const DeviceContext& ctx, const Plan& plan) {
    check(mifft_exec(plan.handle(), x, output, ctx.stream));
}

}  // namespace mifftxx
