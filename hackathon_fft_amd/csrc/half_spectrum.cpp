// half_spectrum.cpp -- passes of the plans with MIFFT_FLAG_HALF_SPECTRUM (numpy rfftn / irfftn; include/mifft.h).
//
// The complex side of such a plan holds h = n / 2 + 1 bins along the last dimension (n = dims[ndim - 1]), so the tensor it
// moves is H = prod / n * h complex per transform.  One launch per dimension, none of the Hermitian / half-store / plane /
// four-step machinery of the full-spectrum schedules:
//   forward   packed real rows (TileCfg::R2C) x -> out at row pitch h, then one in-place column pass per outer dimension
//             on out, its column space counted in h;
//   inverse   the outer dimensions first, as inverse column passes: the first reads x and writes the plan scratch (x is
//             never written, out is too small for H complex), the others run in place on the scratch; then the folded
//             packed rows (TileCfg::C2R) scratch -> out.  A 1-D plan is the single C2R pass x -> out.
// The column kernels are selected exactly as for a complex plan of the half-spectrum shape: every size-dependent choice
// (streaming twins, cache policy, grid) sees the H-complex tensor, not prod complex elements.
#include "mifft_config.h"
#include "mifft_internal.h"

namespace mifft {

namespace {

// the largest outer dimension a single in-place column tile takes here (beyond it the full-spectrum plans route through
// the four-step / FS1 passes and the plan scratch, which this route does not)
constexpr int64_t kMaxColumn = 4096;

// the complex plan of the half-spectrum shape, used only to select the column kernels
Plan half_shape(const Plan& p) {
    Plan q;
    q.device = p.device;
    q.in_dtype = q.out_dtype = p.out_dtype;
    q.ndim = p.ndim;
    for (int i = 0; i < p.ndim; ++i) q.dims[i] = p.dims[i];
    q.dims[p.ndim - 1] = p.dims[p.ndim - 1] / 2 + 1;
    q.batch = p.batch;
    q.sel_batch = p.sel_batch;
    q.prod = p.prod_half;
    q.prod_half = p.prod_half;
    q.in_components = 2;
    q.inverse = p.inverse;
    q.flags = 0;
    q.num_cus = p.num_cus;
    q.cache_resident_nd = p.cache_resident_nd;
    return q;
}

}  // namespace

// checks that need no device: MIFFT_OK, or the status and its reason
int half_spectrum_check(const Plan& p, std::string& why) {
    const int64_t n = p.dims[p.ndim - 1];
    if (p.flags & MIFFT_FLAG_FAITHFUL_STAGES) {
        why = "MIFFT_FLAG_HALF_SPECTRUM with MIFFT_FLAG_FAITHFUL_STAGES: the reference has no half spectrum to be faithful to";
        return MIFFT_ERR_UNSUPPORTED;
    }
    if (p.in_components != (p.inverse ? 2 : 1)) {
        why = p.inverse ? "a half-spectrum inverse reads complex input (in_components = 2)"
                        : "a half-spectrum forward reads real input (in_components = 1)";
        return MIFFT_ERR_BAD_COMPONENTS;
    }
    if (p.inverse && p.in_dtype != p.out_dtype) {
        why = "a half-spectrum inverse reads the plan's own float type (in_dtype == out_dtype)";
        return MIFFT_ERR_BAD_DTYPE;
    }
    if (n % 2 != 0) {
        why = "half spectrum of an odd last dimension (" + std::to_string(n) + ") is not supported";
        return MIFFT_ERR_UNSUPPORTED;
    }
    for (int i = 0; i + 1 < p.ndim; ++i)
        if (!p.kept(i) && p.dims[i] > kMaxColumn) {
            why = "half spectrum: dimension " + std::to_string(i) + " (" + std::to_string(p.dims[i]) +
                  " points) is longer than one column tile (" + std::to_string(kMaxColumn) + ")";
            return MIFFT_ERR_UNSUPPORTED;
        }
    std::string w;
    if (!tile_family_supported(TileFamily::HalfRows, p, n, 1, w)) {
        why = "half spectrum of a last dimension of " + std::to_string(n) + " points: " + w;
        return MIFFT_ERR_UNSUPPORTED;
    }
    return MIFFT_OK;
}

int build_half_spectrum(Plan& p, const std::vector<std::vector<uint32_t>>& ordered,
                        const std::vector<std::vector<uint32_t>>& processed, std::string& why) {
    const int nd = p.ndim;
    const int64_t n = p.dims[nd - 1], h = n / 2 + 1;
    const Config& cfg = config();
    {   // the Infinity-Cache policy of mifft_plan_create, on the bytes this plan's complex side really has
        const double bytes = p.size_batch() * (double)p.prod_half * (double)p.out_elem_bytes();
        p.cache_resident_nd = nd >= 2 && (cfg.nd_mode & 1) && bytes <= cfg.nd_out_max_bytes && bytes >= cfg.nd_out_min_bytes;
    }
    const Plan q = half_shape(p);

    auto add = [&](DimPass& ps) -> int {
        if (ps.prepare) {
            const int rc = ps.prepare();
            if (rc) return rc;
        }
        const hipError_t e = ps.r2c || ps.c2r ? upload_packed_tables(p.out_dtype, p.inverse != 0, ps)
                                              : upload_twiddle_table(p.out_dtype, ps.N, p.inverse != 0, &ps.d_twiddle);
        return append_pass(p, ps, e, "twiddle table upload");
    };
    auto rows = [&](DimPass& ps) -> int {
        ps.dim_index = nd - 1;
        ps.N = n;
        ps.inner = 1;
        ps.outer = p.prod / n;
        ps.radices = ordered[nd - 1];
        ps.processed = processed[nd - 1];
        ps.half_pitch = h;
        if (!select_tile_family(TileFamily::HalfRows, p, ps, why)) return MIFFT_ERR_UNSUPPORTED;
        return add(ps);
    };
    auto column = [&](int j, DimPass& ps) -> int {
        ps.dim_index = j;
        ps.N = p.dims[j];
        ps.inner = h;
        for (int k = j + 1; k < nd - 1; ++k) ps.inner *= p.dims[k];
        ps.outer = 1;
        for (int k = 0; k < j; ++k) ps.outer *= p.dims[k];
        ps.radices = ordered[j];
        ps.processed = processed[j];
        std::string whyj;
        if (!select_fast(q, ps) && !select_jit(q, ps, whyj)) {
            why = "half spectrum: no column kernel for dimension " + std::to_string(j) + " (" + std::to_string(ps.N) +
                  " points" + (whyj.empty() ? "" : ": " + whyj) + ")";
            return MIFFT_ERR_UNSUPPORTED;
        }
        return add(ps);
    };

    int rc = MIFFT_OK;
    if (!p.inverse) {
        DimPass r;
        r.first = true;
        rc = rows(r);
        for (int j = nd - 2; j >= 0 && rc == MIFFT_OK; --j) {
            if (p.kept(j)) continue;  // (MIFFT_FLAG_KEEP_DIM: carried through, counted in the inner / outer of the others)
            DimPass c;  // in place on out
            rc = column(j, c);
        }
    } else {
        int ncols = 0;  // column passes (the dimensions before the last one that are not kept)
        for (int j = 0; j + 1 < nd; ++j) ncols += p.kept(j) ? 0 : 1;
        if (ncols > 0) {
            p.scratch_bytes = (size_t)p.batch * p.scratch_row_bytes();
            if (p.scratch_bytes > 0) {
                const hipError_t e = hipMalloc(&p.d_scratch, p.scratch_bytes);
                if (e != hipSuccess) {
                    p.d_scratch = nullptr;
                    p.scratch_bytes = 0;
                    return hip_error(e, "half-spectrum scratch");
                }
            }
        }
        bool from_x = true;
        for (int j = nd - 2; j >= 0 && rc == MIFFT_OK; --j) {
            if (p.kept(j)) continue;
            DimPass c;
            c.src_buf = from_x ? 0 : 2;  // x -> scratch, then in place on the scratch
            c.dst_buf = 2;
            from_x = false;
            rc = column(j, c);
        }
        if (rc == MIFFT_OK) {
            DimPass r;
            r.first = ncols == 0;
            r.src_buf = ncols == 0 ? 0 : 2;
            r.dst_buf = 1;
            rc = rows(r);
        }
    }
    if (rc != MIFFT_OK) return rc;
    if (cfg.nd_mode & 2) {  // in-place passes alternate their walking direction (bit-identical results)
        int k = 0;
        for (DimPass& ps : p.passes) {
            const bool in_place = (ps.src_buf < 0 && !ps.first) || (ps.src_buf == 2 && ps.dst_buf == 2);
            if (in_place) ps.reverse = (k++ % 2) == 0;
        }
    }
    return MIFFT_OK;
}

}  // namespace mifft
