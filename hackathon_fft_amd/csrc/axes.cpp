// axes.cpp -- passes of the plans with a keep bit (MIFFT_FLAG_KEEP_DIM: numpy `axes=`, torch `dim=`; include/mifft.h).
//
// A kept dimension is carried through like an extra batch dimension.  One launch per TRANSFORMED dimension, innermost first:
// the first reads x and writes out, the others run in place on out.  The pass over dimension i is an (N, inner, outer)
// pass with inner = prod(dims after i) and outer = prod(dims before i), kept or not.  Kernel per pass, by its stride
// I = inner (complex elements):
//   I == 1                  the row selection of full plans (tuned table, runtime specialisation);
//   I * elem_bytes >= 128   the column tiles (the first pass reads x out of place, real / foreign input specialised at run
//                           time through TileCfg::IN_REAL / IT);
//   I * elem_bytes <  128   the interleaved block tile (TileCfg::ILV, select_jit_ilv) when one N x I block fits its LDS,
//                           else the column tiles, whose tiles are then narrower than a 128-B line;
// and the literal-stage family (kernels_generic.hip) for a length without a fused configuration or under MIFFT_JIT=0.
// None of the plane / four-step / Hermitian / half-store routes of the full plans: those are refused with a reason.
// Half-spectrum plans with a mask go through build_half_spectrum, which skips the kept dimensions.
#include "mifft_config.h"
#include "mifft_internal.h"

namespace mifft {

namespace {

// the longest strided dimension one in-place column tile takes (beyond it full plans route through the plan scratch)
constexpr int64_t kMaxStrided = 4096;

// the element bytes from which a stride makes whole 128-B lines of a column tile
constexpr int64_t kLineBytes = 128;

}  // namespace

// checks that need no device: MIFFT_OK, or the status and its reason
int axes_check(const Plan& p, std::string& why) {
    const int nd = p.ndim;
    const bool f64 = p.out_dtype == MIFFT_F64;
    if (p.half_spectrum() && p.kept(nd - 1)) {
        why = "MIFFT_FLAG_HALF_SPECTRUM with the last dimension kept: numpy halves the last TRANSFORMED axis, which would be "
              "strided here";
        return MIFFT_ERR_UNSUPPORTED;
    }
    for (int i = 0; i < nd; ++i) {
        if (p.kept(i)) continue;
        const bool innermost = i == nd - 1;
        // (a half-spectrum plan's last dimension is checked by half_spectrum_check: packed real rows)
        if (innermost && p.half_spectrum()) continue;
        const int64_t lim = innermost ? (f64 ? 8192 : 16384) : kMaxStrided;
        if (p.dims[i] > lim) {
            why = "dimension " + std::to_string(i) + " (" + std::to_string(p.dims[i]) + " points) of a plan with kept "
                  "dimensions is longer than " + (innermost ? "one single-launch row (" : "one column tile (") +
                  std::to_string(lim) + "): masked plans have no four-step or transposed routes";
            return MIFFT_ERR_UNSUPPORTED;
        }
    }
    return MIFFT_OK;
}

int build_axes(Plan& p, const std::vector<std::vector<uint32_t>>& ordered,
               const std::vector<std::vector<uint32_t>>& processed, std::string& why) {
    if (p.half_spectrum()) return build_half_spectrum(p, ordered, processed, why);
    const int nd = p.ndim;
    const Config& cfg = config();
    const int64_t esz = (int64_t)p.out_elem_bytes();
    bool first = true;
    for (int i = nd - 1; i >= 0; --i) {
        if (p.kept(i)) continue;
        DimPass ps;
        ps.dim_index = i;
        ps.N = p.dims[i];
        ps.inner = 1;
        for (int k = i + 1; k < nd; ++k) ps.inner *= p.dims[k];
        ps.outer = 1;
        for (int k = 0; k < i; ++k) ps.outer *= p.dims[k];
        ps.radices = ordered[i];
        ps.processed = processed[i];
        ps.first = first;
        if (first) {  // x -> out
            ps.src_buf = 0;
            ps.dst_buf = 1;
        }
        std::string whyj, whyi, whyg;
        bool ok = false;
        if (ps.inner == 1) {
            ok = select_fast(p, ps) || select_jit(p, ps, whyj);
        } else {
            if (ps.inner * esz < kLineBytes && cfg.ilv) ok = select_jit_ilv(p, ps, whyi);
            if (!ok) ok = select_fast(p, ps) || select_jit(p, ps, whyj);
        }
        if (!ok) ok = select_generic(p, ps, whyg);
        if (!ok) {
            why = "dimension " + std::to_string(i) + " (" + std::to_string(ps.N) + " points at stride " +
                  std::to_string((long long)ps.inner) + ") of a plan with kept dimensions has no kernel" +
                  (whyj.empty() ? "" : ": " + whyj) + (whyg.empty() ? "" : "; literal stages: " + whyg);
            return MIFFT_ERR_UNSUPPORTED;
        }
        if (ps.prepare) {
            const int rc = ps.prepare();
            if (rc) return rc;
        }
        const hipError_t e = upload_twiddle_table(p.out_dtype, ps.N, p.inverse != 0, &ps.d_twiddle);
        p.passes.push_back(ps);
        if (e != hipSuccess) return hip_error(e, "twiddle table upload");
        first = false;
    }
    if (cfg.nd_mode & 2) {  // in-place passes alternate their walking direction (bit-identical results)
        int k = 0;
        for (DimPass& ps : p.passes)
            if (!ps.first) ps.reverse = (k++ % 2) == 0;
    }
    return MIFFT_OK;
}

}  // namespace mifft
