// dct.cpp -- the plans with MIFFT_FLAG_DCT (scipy.fft.dct / idct of type 2 over real rows; include/mifft.h).
//
// One launch, no scratch: the packed real-row kernel of the row length with TileCfg::DCT set.  The forward (DCT-II) is an R2C
// tile whose load applies Makhoul's even / odd permutation on the LDS side and whose unpacking loop multiplies by the
// quarter-sample twiddle W_4n^k and stores reals; the inverse is the mirror on a C2R tile (tile_kernel.h, TileCfg::DCT).  Both
// sides of the plan are (batch, n, 1) real tensors, so every size-dependent choice sees batch * n real elements.
//
// A plan whose `bases` start with MIFFT_DCT_TYPE4_TAG (Plan::dct4) is a DCT-IV: a complex row tile of n / 2 points between the
// twiddles p_m = e^(-i pi (8m+1) / 8n), the same kernel in both directions with another scale (TileCfg::DCT = 4).
//
// A plan tagged with MIFFT_DST_TAG or MIFFT_DST_TYPE4_TAG (Plan::dst) is the sine transform of the same type: the same pass,
// tables and scales, and a kernel with TileCfg::DST set (kernels_jit.cpp takes the bit from the plan; compiled at run time only).
#include <cmath>

#include "mifft_config.h"
#include "mifft_internal.h"

namespace mifft {

// checks that need no device: MIFFT_OK, or the status and its reason
int dct_check(const Plan& p, std::string& why) {
    if (p.flags & MIFFT_FLAG_HALF_SPECTRUM) {
        why = "MIFFT_FLAG_DCT with MIFFT_FLAG_HALF_SPECTRUM: a DCT has no half spectrum";
        return MIFFT_ERR_UNSUPPORTED;
    }
    if (p.flags & MIFFT_FLAG_FAITHFUL_STAGES) {
        why = "MIFFT_FLAG_DCT with MIFFT_FLAG_FAITHFUL_STAGES: the reference has no DCT to be faithful to";
        return MIFFT_ERR_UNSUPPORTED;
    }
    if (p.flags & MIFFT_FLAG_KEEP_MASK) {
        why = "MIFFT_FLAG_DCT with MIFFT_FLAG_KEEP_DIM: a DCT plan transforms its one dimension";
        return MIFFT_ERR_UNSUPPORTED;
    }
    if (p.in_components != 1) {
        why = "a DCT reads and writes real rows (in_components = 1)";
        return MIFFT_ERR_BAD_COMPONENTS;
    }
    if (p.ndim != 1) {
        why = "MIFFT_FLAG_DCT transforms the rows of a (batch, n, 1) tensor: ndim must be 1, not " + std::to_string(p.ndim);
        return MIFFT_ERR_UNSUPPORTED;
    }
    if (p.dct4 && p.in_dtype != p.out_dtype) {
        why = "a DCT-IV reads the plan's own float type in both directions (in_dtype == out_dtype)";
        return MIFFT_ERR_BAD_DTYPE;
    }
    if (p.inverse && p.in_dtype != p.out_dtype) {
        why = "an inverse DCT reads the plan's own float type (in_dtype == out_dtype)";
        return MIFFT_ERR_BAD_DTYPE;
    }
    const int64_t n = p.dims[0];
    if (n % 2 != 0) {
        why = "DCT of an odd length (" + std::to_string(n) + ") is not supported";
        return MIFFT_ERR_UNSUPPORTED;
    }
    if (n < 8) {
        why = "DCT of fewer than 8 points (" + std::to_string(n) + ") is not supported";
        return MIFFT_ERR_UNSUPPORTED;
    }
    std::string w;
    if (p.dct4) {
        if (!tile_family_supported(TileFamily::Dct4Rows, p, n, 1, w)) {
            why = "DCT-IV of " + std::to_string(n) + " points: " + w;
            return MIFFT_ERR_UNSUPPORTED;
        }
        return MIFFT_OK;
    }
    if (!tile_family_supported(TileFamily::DctRows, p, n, 1, w)) {
        why = "DCT of " + std::to_string(n) + " points: " + w;
        return MIFFT_ERR_UNSUPPORTED;
    }
    return MIFFT_OK;
}

// W_4n^k = e^(-2 pi i k / 4n), k = 0 .. n / 2, evaluated in long double and rounded once
template <typename T>
static hipError_t upload_quarter_table_t(int64_t n, void** d_table) {
    const long double half_pi = 1.570796326794896619231321691639751442L;
    std::vector<T> tab((size_t)(n / 2 + 1) * 2);
    for (int64_t k = 0; k <= n / 2; ++k) {
        const long double th = -half_pi * (long double)k / (long double)n;
        tab[2 * k] = (T)cosl(th);
        tab[2 * k + 1] = (T)sinl(th);
    }
    hipError_t e = hipMalloc(d_table, tab.size() * sizeof(T));
    if (e == hipSuccess) e = hipMemcpy(*d_table, tab.data(), tab.size() * sizeof(T), hipMemcpyHostToDevice);
    return e;
}

hipError_t upload_quarter_table(int out_dtype, int64_t n, void** d_table) {
    return out_dtype == MIFFT_F64 ? upload_quarter_table_t<double>(n, d_table) : upload_quarter_table_t<float>(n, d_table);
}

// p_m = e^(-i pi (8m+1) / 8n), m = 0 .. n / 2 - 1: the pre- and the post-twiddle of a DCT-IV of n points, evaluated in long
// double and rounded once
template <typename T>
static hipError_t upload_dct4_table_t(int64_t n, void** d_table) {
    const long double pi = 3.141592653589793238462643383279502884L;
    std::vector<T> tab((size_t)(n / 2) * 2);
    for (int64_t m = 0; m < n / 2; ++m) {
        const long double th = -pi * (long double)(8 * m + 1) / (long double)(8 * n);
        tab[2 * m] = (T)cosl(th);
        tab[2 * m + 1] = (T)sinl(th);
    }
    hipError_t e = hipMalloc(d_table, tab.size() * sizeof(T));
    if (e == hipSuccess) e = hipMemcpy(*d_table, tab.data(), tab.size() * sizeof(T), hipMemcpyHostToDevice);
    return e;
}

hipError_t upload_dct4_table(int out_dtype, int64_t n, void** d_table) {
    return out_dtype == MIFFT_F64 ? upload_dct4_table_t<double>(n, d_table) : upload_dct4_table_t<float>(n, d_table);
}

// the one scale of a DCT-IV: X = 2 sum, "ortho" times sqrt(1 / 2n) in both directions; the plain inverse divides by 2n
static double dct4_scale(int64_t n, bool inverse, bool ortho) {
    const long double dn = (long double)n;
    return (double)(ortho ? 2.0L * sqrtl(1.0L / (2.0L * dn)) : inverse ? 1.0L / dn : 2.0L);
}

// the DCT-IV pass of n points over `outer` rows per batch entry: kernel, scale and tables; appended to plan.passes
static int build_dct4_rows(Plan& p, const std::vector<uint32_t>& ordered, const std::vector<uint32_t>& processed, std::string& why) {
    const int64_t n = p.dims[0];
    DimPass ps = fused_row_pass(0, n, 1, ordered, processed, /*half_pitch=*/false);
    if (!select_tile_family(TileFamily::Dct4Rows, p, ps, why)) return MIFFT_ERR_UNSUPPORTED;
    ps.dct_s0 = ps.dct_s1 = dct4_scale(n, p.inverse != 0, (p.flags & MIFFT_FLAG_DCT_ORTHO) != 0);
    // the passes run n / 2 points, forward in both directions
    hipError_t e = upload_twiddle_table(p.out_dtype, n / 2, false, &ps.d_twiddle);
    if (e == hipSuccess) e = upload_dct4_table(p.out_dtype, n, &ps.d_aux2);
    return append_pass(p, ps, e, "DCT-IV table upload");
}

// the scales of bin 0 and of the other bins.  Forward: X[k] = 2 Re(..), "ortho" times sqrt(1 / 4n) and sqrt(1 / 2n).
// Inverse: the bins are scaled as they are loaded -- the half of V[k] = conj(W) (X[k] - i X[n-k]) / 2, the 1 / n of the
// n-point inverse, and "ortho" undone (times sqrt(4n) and sqrt(2n)).
void dct_scales(int64_t n, bool inverse, bool ortho, double& s0, double& s1) {
    const long double dn = (long double)n;
    if (!inverse) {
        s0 = (double)(ortho ? 2.0L * sqrtl(1.0L / (4.0L * dn)) : 2.0L);
        s1 = (double)(ortho ? 2.0L * sqrtl(1.0L / (2.0L * dn)) : 2.0L);
    } else {
        s0 = (double)(ortho ? sqrtl(4.0L * dn) / (2.0L * dn) : 1.0L / (2.0L * dn));
        s1 = (double)(ortho ? sqrtl(2.0L * dn) / (2.0L * dn) : 1.0L / (2.0L * dn));
    }
}

// the packed-row pass of n points over `outer` rows per batch entry (the one pass of a MIFFT_FLAG_DCT plan, the first pass
// of an N-D DCT plan whose last dimension is transformed): kernel, scales and tables; appended to plan.passes
int build_dct_rows(Plan& p, int dim_index, int64_t outer, const std::vector<uint32_t>& ordered,
                   const std::vector<uint32_t>& processed, std::string& why) {
    const int64_t n = p.dims[dim_index];
    // (half_pitch: unused by the DCT loads and stores, both sides are rows of n reals)
    DimPass ps = fused_row_pass(dim_index, n, outer, ordered, processed, /*half_pitch=*/true);
    if (!select_tile_family(TileFamily::DctRows, p, ps, why)) return MIFFT_ERR_UNSUPPORTED;
    dct_scales(n, p.inverse != 0, (p.flags & MIFFT_FLAG_DCT_ORTHO) != 0, ps.dct_s0, ps.dct_s1);
    hipError_t e = upload_packed_tables(p.out_dtype, p.inverse != 0, ps);
    if (e == hipSuccess) e = upload_quarter_table(p.out_dtype, n, &ps.d_aux2);  // the DCT twiddle W_4n^k
    return append_pass(p, ps, e, "DCT table upload");
}

int build_dct(Plan& p, const std::vector<uint32_t>& ordered, const std::vector<uint32_t>& processed, std::string& why) {
    if (p.dct4) return build_dct4_rows(p, ordered, processed, why);
    return build_dct_rows(p, 0, 1, ordered, processed, why);
}

}  // namespace mifft
