// dctn.cpp -- the plans with MIFFT_FLAG_DCT_ND (scipy.fft.dctn / idctn of type 2 over real tensors; include/mifft.h).
//
// Both sides are real (batch, d0.., 1) tensors of one shape.  An N-D DCT is separable and its 1-D factors commute, so every
// plan, forward or inverse, runs one launch per TRANSFORMED dimension, innermost first: the first reads x and writes out, the
// others run in place on out; no scratch.  A kept dimension (MIFFT_FLAG_KEEP_DIM) is carried through like a batch dimension.
//   last dimension   the packed-row kernel of a MIFFT_FLAG_DCT plan (dct.cpp, TileCfg::DCT on R2C / C2R) over prod / n rows;
//   other dimension  n points at a stride of S reals, S = the product of the extents after it, even: the same memory viewed
//                    as complex elements at stride S / 2 is PAIRS of adjacent real columns, u = x_a + i x_b, and the in-place
//                    column tile moves them coalesced.  TileCfg::DCT on a column configuration (tile_kernel.h) permutes,
//                    transforms and separates (forward) or combines, transforms and un-permutes (inverse) such a pair.
// A plan tagged with MIFFT_DST_TAG (Plan::dst) runs the DST-II / its inverse along every transformed dimension: the same
// passes, tables and scales, every kernel with TileCfg::DST set (kernels_jit.cpp takes the bit from the plan).
#include "mifft_config.h"
#include "mifft_internal.h"

namespace mifft {

namespace {

constexpr int64_t kMaxColumn = 4096;  // the longest dimension of one in-place column tile (as the masked plans, axes.cpp)

// reals after dimension i: the stride of its points
int64_t stride_reals(const Plan& p, int i) {
    int64_t s = 1;
    for (int k = i + 1; k < p.ndim; ++k) s *= p.dims[k];
    return s;
}

}  // namespace

// checks that need no device: MIFFT_OK, or the status and its reason
int dctn_check(const Plan& p, std::string& why) {
    if (p.flags & MIFFT_FLAG_DCT) {
        why = "MIFFT_FLAG_DCT together with MIFFT_FLAG_DCT_ND: one request or the other";
        return MIFFT_ERR_UNSUPPORTED;
    }
    if (p.flags & MIFFT_FLAG_HALF_SPECTRUM) {
        why = "MIFFT_FLAG_DCT_ND with MIFFT_FLAG_HALF_SPECTRUM: a DCT has no half spectrum";
        return MIFFT_ERR_UNSUPPORTED;
    }
    if (p.flags & MIFFT_FLAG_FAITHFUL_STAGES) {
        why = "MIFFT_FLAG_DCT_ND with MIFFT_FLAG_FAITHFUL_STAGES: the reference has no DCT to be faithful to";
        return MIFFT_ERR_UNSUPPORTED;
    }
    if (p.in_components != 1) {
        why = "a DCT reads and writes real tensors (in_components = 1)";
        return MIFFT_ERR_BAD_COMPONENTS;
    }
    if (p.inverse && p.in_dtype != p.out_dtype) {
        why = "an inverse DCT reads the plan's own float type (in_dtype == out_dtype)";
        return MIFFT_ERR_BAD_DTYPE;
    }
    const int nd = p.ndim;
    bool first = true;
    for (int i = nd - 1; i >= 0; --i) {
        if (p.kept(i)) continue;
        const int64_t n = p.dims[i];
        const std::string dim = "dimension " + std::to_string(i) + " (" + std::to_string(n) + " points)";
        if (i == nd - 1) {  // the packed-row kernel and its limits (dct.cpp)
            if (n % 2 != 0) {
                why = "DCT of an odd last " + dim + " is not supported";
                return MIFFT_ERR_UNSUPPORTED;
            }
            if (n < 8) {
                why = "DCT of a last " + dim + " of fewer than 8 points is not supported";
                return MIFFT_ERR_UNSUPPORTED;
            }
            std::string w;
            if (!tile_family_supported(TileFamily::DctRows, p, n, 1, w)) {
                why = "DCT of the last " + dim + ": " + w;
                return MIFFT_ERR_UNSUPPORTED;
            }
        } else {
            const int64_t s = stride_reals(p, i);
            if (s % 2 != 0) {
                why = dim + " has an odd stride of " + std::to_string((long long)s) + " reals: the column pass transforms "
                      "pairs of adjacent real columns";
                return MIFFT_ERR_UNSUPPORTED;
            }
            if (s == 2) {
                why = dim + " has a stride of 2 reals (a trailing extent of 2): a single pair of columns is a row-shaped "
                      "problem, not supported";
                return MIFFT_ERR_UNSUPPORTED;
            }
            if (n > kMaxColumn) {
                why = dim + " is longer than one column tile (" + std::to_string((long long)kMaxColumn) + ")";
                return MIFFT_ERR_UNSUPPORTED;
            }
            if (first && p.in_dtype != p.out_dtype) {
                why = "the first pass of this plan is the column pass over " + dim + ", which reads the plan's own float "
                      "type (in_dtype == out_dtype): only a transformed last dimension widens a foreign in_dtype";
                return MIFFT_ERR_UNSUPPORTED;
            }
            std::string w;
            if (!tile_family_supported(TileFamily::DctCols, p, n, s / 2, w)) {
                why = "DCT column pass over " + dim + ": " + w;
                return MIFFT_ERR_UNSUPPORTED;
            }
        }
        first = false;
    }
    return MIFFT_OK;
}

int build_dctn(Plan& p, const std::vector<std::vector<uint32_t>>& ordered,
               const std::vector<std::vector<uint32_t>>& processed, std::string& why) {
    const int nd = p.ndim;
    const bool ortho = (p.flags & MIFFT_FLAG_DCT_ORTHO) != 0;
    bool first = true;
    for (int i = nd - 1; i >= 0; --i) {
        if (p.kept(i)) continue;
        const int64_t n = p.dims[i];
        if (i == nd - 1) {
            const int rc = build_dct_rows(p, i, p.prod / n, ordered[i], processed[i], why);
            if (rc) return rc;
            first = false;
            continue;
        }
        DimPass ps;
        ps.dim_index = i;
        ps.N = n;
        ps.inner = stride_reals(p, i) / 2;  // pairs of real columns
        ps.outer = 1;
        for (int k = 0; k < i; ++k) ps.outer *= p.dims[k];
        ps.radices = ordered[i];
        ps.processed = processed[i];
        ps.first = first;
        std::string w;
        if (!select_tile_family(TileFamily::DctCols, p, ps, w)) {
            why = "DCT column pass over dimension " + std::to_string(i) + " (" + std::to_string(n) + " points): " + w;
            return MIFFT_ERR_UNSUPPORTED;
        }
        dct_scales(n, p.inverse != 0, ortho, ps.dct_s0, ps.dct_s1);
        // the n-point passes, and the quarter-sample twiddle W_4n^k of the separating store / combining load
        hipError_t e = upload_twiddle_table(p.out_dtype, n, p.inverse != 0, &ps.d_twiddle);
        if (e == hipSuccess) e = upload_quarter_table(p.out_dtype, n, &ps.d_aux2);
        if (const int rc = append_pass(p, ps, e, "DCT table upload")) return rc;
        first = false;
    }
    if (config().nd_mode & 2) {  // in-place passes alternate their walking direction (bit-identical results)
        int k = 0;
        for (DimPass& ps : p.passes)
            if (!ps.first) ps.reverse = (k++ % 2) == 0;
    }
    return MIFFT_OK;
}

}  // namespace mifft
