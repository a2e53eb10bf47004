// schedule.cpp -- the general route of plan creation: the passes of a full transform over every dimension.
//
// Host scheduler replacing _run_gpu_nd_fft (fft/fft/_ndim_fft_gpu.mojo:462-642): the contiguous (last) dimension is
// transformed first, reading `x` and writing `out`; every earlier dimension is then transformed IN PLACE on `out` by a
// strided tile kernel.  The reference's transpose launches and scratch buffer do not exist here: d launches instead of
// d + 2(d-1).  One kernel per pass, chosen by the cascade of Scheduler::select_pass.
#include "mifft_config.h"
#include "mifft_internal.h"

namespace mifft {

// Frees and nulls the four device tables of a pass.  A candidate pass that plan creation drops again has been through
// selectors only: d_twiddle and d_aux3 are filled after selection (upload_twiddles; the four-step builders, which free their
// own passes), so there this frees what a selector may upload -- the Rader tables in d_aux / d_aux2.  (File-local: the
// four-step builders keep a copy of their own under the same name, kernels_fourstep.hip.)
static void free_pass_tables(DimPass& ps) {
    if (ps.d_twiddle) (void)hipFree(ps.d_twiddle);
    if (ps.d_aux) (void)hipFree(ps.d_aux);
    if (ps.d_aux2) (void)hipFree(ps.d_aux2);
    if (ps.d_aux3) (void)hipFree(ps.d_aux3);
    ps.d_twiddle = ps.d_aux = ps.d_aux2 = ps.d_aux3 = nullptr;
}

void free_plan_device(Plan& p) {
    for (auto& ps : p.passes) free_pass_tables(ps);
    if (p.d_scratch) (void)hipFree(p.d_scratch);
    p.d_scratch = nullptr;
}

namespace {

// What the cascade reports for one dimension.  Selected: `ps` has its kernel; the caller prepares it, uploads its tables and
// pushes it.  Appended: a route builder pushed its own passes.  Failed: Scheduler::status (and `why`).  None is the
// cascade's own "not yet" and never leaves select_pass.
enum class Outcome { None, Selected, Appended, Failed };

struct Scheduler {
    Plan& p;
    const Config& cfg;
    const std::vector<std::vector<uint32_t>>& ordered;
    const std::vector<std::vector<uint32_t>>& processed;
    int herm_known = -1;  // the memo of last_pass_will_be_hermitian(), per schedule attempt: -1 = not asked yet
    // Half-spectrum schedule of a real-input plan with exactly one pass between the first and the last (rows / columns /
    // columns of a 3-D plan, plane / columns / columns of a 4-D one): the FIRST pass stores only the lower half of the dimension
    // it transforms last (dims[2]), the middle pass transforms only those columns, the Hermitian last pass halves that same
    // dimension (Plan::herm_axis = 2) -- every pass but the last moves half the tensor.  allow_first_axis: this attempt may
    // start it; first_axis: it has.  When a kernel is missing, build_general falls back to herm_axis = 1.
    bool allow_first_axis = false, first_axis = false;
    int status = MIFFT_OK;  // of Outcome::Failed; MIFFT_ERR_HIP has been recorded where it arose, any other has `why`
    std::string why;

    bool herm_possible() const {
        return cfg.herm != 0 && cfg.half_store && p.ndim >= 2 && p.ndim <= 4 && p.in_components == 1 &&
               !(p.flags & MIFFT_FLAG_FAITHFUL_STAGES);
    }

    // the pass over dimension i before any selection
    DimPass pass_of(int i) const {
        DimPass ps;
        ps.dim_index = i;
        ps.N = p.dims[i];
        for (int k = i + 1; k < p.ndim; ++k) ps.inner *= p.dims[k];
        for (int k = 0; k < i; ++k) ps.outer *= p.dims[k];
        ps.radices = ordered[i];
        ps.processed = processed[i];
        ps.first = i == p.ndim - 1;
        return ps;
    }

    // a Hermitian twin for the last pass: a tuned one first, else the runtime-specialised one
    bool select_herm(DimPass& ps) const {
        ps.herm_only = true;
        bool ok = select_fast(p, ps);
        ps.herm_only = false;
        if (!ok && ps.N <= 4096) {
            std::string whyh;
            ok = select_jit(p, ps, whyh) && ps.herm_d2 > 0;
        }
        return ok;
    }

    // Will the LAST pass (dimension 0) be a Hermitian twin?  Asked when the pass over dimension 1 is selected: that pass may
    // then store only the lower half of its dimension (TileCfg::HS).  The same selection select_pass makes for i == 0, on a
    // scratch DimPass (whatever it uploads is freed again); build_general checks at the end that both agree.  Asked ONCE per
    // attempt, after p.hs_selected has been set: a half-store pass in front widens the cases in which the twin pays.
    bool last_pass_will_be_hermitian() {
        if (herm_known >= 0) return herm_known != 0;
        herm_known = 0;
        if (!herm_possible()) return false;
        DimPass t = pass_of(0);
        t.first = false;
        if (t.inner >= (1ll << 30)) return false;
#ifdef MIFFT_EXPERIMENTAL  // (lab knob that sends long strided dimensions to the four-step before anything else)
        if (cfg.fs_strided_min_n > 0 && t.N >= cfg.fs_strided_min_n) return false;
#endif
        t.want_herm = true;
        const bool ok = select_herm(t);
        free_pass_tables(t);
        herm_known = ok ? 1 : 0;
        return ok;
    }

    // t: the first pass with a half-store kernel selected (`found`).  Commits the plan to the half-spectrum schedule when the
    // last pass will be a Hermitian twin under it; else restores the plan and frees t's tables.
    bool try_first_axis(DimPass& t, bool found) {
        if (!found) return false;
        p.herm_axis = 2;
        p.hs_selected = true;
        herm_known = -1;
        if (last_pass_will_be_hermitian()) return true;
        p.herm_axis = 1;
        p.hs_selected = false;
        herm_known = -1;  // (asked again, for the other schedule, when the pass over dimension 1 is selected)
        free_pass_tables(t);
        return false;
    }

    // A half-store kernel (TileCfg::HS) for pass `t` (= `ps` with want_half and store_lim set): the lab's packed real rows (a
    // measured tie with the tuned half-store kernels; row passes only), else a table twin, else a runtime-specialised one --
    // unless the ordinary table entry is one tuned for a size regime (a non-temporal twin), which is not traded for it:
    // 64 x 1024^2 0.372 -> 0.422 ms with `rows1024_16x8x8_hs_r_jit` in place of `rows1024_16x8x8_r_nt`
    bool select_half_store(const DimPass& ps, DimPass& t) const {
#ifdef MIFFT_EXPERIMENTAL
        std::string whyr;
        if (cfg.r2c_rows && ps.first && select_jit_r2c(p, t, whyr)) return true;
#endif
        if (select_fast(p, t)) return true;
        if (ps.N > 4096) return false;
        DimPass u = ps;
        const bool tuned = select_fast(p, u) && u.regime_twin;
        std::string whyh;
        return !tuned && select_jit(p, t, whyh);
    }

    hipError_t upload_twiddles(DimPass& ps) const {
        const bool inv = p.inverse != 0;
        if (ps.r2c) return upload_packed_tables(p.out_dtype, inv, ps);  // (the lab's packed real rows)
        // (four-step rows inside LDS: the table of the row side, M / N1 points; the column side's goes to d_aux when it
        //  differs, the M-entry table to d_aux3)
        hipError_t e = upload_twiddle_table(p.out_dtype, ps.row2d_m > 0 ? ps.row2d_m / ps.N1 : ps.N, inv, &ps.d_twiddle);
        if (e == hipSuccess && ps.plane_needs_tw1) e = upload_twiddle_table(p.out_dtype, ps.N1, inv, &ps.d_aux);
        if (e == hipSuccess && ps.row2d_m > 0) e = upload_twiddle_table(p.out_dtype, ps.row2d_m, false, &ps.d_aux3);
        if (e == hipSuccess && ps.needs_counters) {  // 16 per-launch counters + the sticky error word
            e = hipMalloc(&ps.d_aux2, 20 * sizeof(unsigned));
            if (e == hipSuccess) e = hipMemset(ps.d_aux2, 0, 20 * sizeof(unsigned));
        }
        return e;
    }

    // The two innermost dimensions (i = ndim - 1 and i - 1) fused in one LDS plane; `ps` becomes that pass.
    bool select_plane(int i, DimPass& ps) {
        DimPass pl = ps;
        pl.dim_index2 = i - 1;
        pl.N1 = p.dims[i - 1];
        pl.outer = 1;
        for (int k = 0; k < i - 1; ++k) pl.outer *= p.dims[k];
        std::string whyp;
        bool fused = false;
        if (allow_first_axis && p.ndim == 4 && herm_possible()) {  // plane / columns / columns: halve the plane's column side
            DimPass t = pl;
            t.want_half = true;
            t.store_lim = (int)(p.dims[2] / 2);
            if (try_first_axis(t, select_fast_plane(p, t) || select_jit_plane(p, t, whyp))) {
                pl = t;
                fused = first_axis = true;
            }
        }
        if (!fused && i - 1 == 1 && herm_possible()) {  // the plane's column side is dimension 1: half store
            DimPass t = pl;
            t.want_half = true;
            t.store_lim = (int)(p.dims[1] / 2);
            p.hs_selected = select_fast_plane(p, t) || select_jit_plane(p, t, whyp);
            fused = p.hs_selected && last_pass_will_be_hermitian();
            if (fused) pl = t;
            p.hs_selected = fused;
        }
        if (!fused) fused = select_fast_plane(p, pl) || select_jit_plane(p, pl, whyp);
#ifdef MIFFT_EXPERIMENTAL  // L2-resident image kernel: a documented negative result, lab builds only
        if (!fused) fused = select_jit_image(p, pl, whyp);
#endif
        if (fused) ps = pl;
        return fused;
    }

    // What a route builder made of the dimension: its passes are appended, or it ran out of device memory -- an error, not a
    // reason to try a slower kernel -- or it has no route for it (None: the cascade goes on).
    Outcome routed(bool built, const std::string& prefix, const std::string& why_not) {
        if (built) return Outcome::Appended;
        if (!p.alloc_failed) return Outcome::None;
        status = set_error(MIFFT_ERR_HIP, prefix + why_not);
        return Outcome::Failed;
    }

    // The cascade for dimension i.  A fused plane also covers dimension i - 1 and decrements i.
    Outcome select_pass(int& i, DimPass& ps) {
        const int ndim = p.ndim;
        const std::string strided_prefix = "four-step of strided dimension " + std::to_string(i) + ": ";
        if (!(p.flags & MIFFT_FLAG_FAITHFUL_STAGES)) {
            if (i == ndim - 1 && ndim >= 2 && select_plane(i, ps)) {
                --i;  // dimension i-1 is covered by this pass
                return Outcome::Selected;
            }
            // rows / columns / columns of a real-input 3-D plan: the row pass stores the lower half of every row
            if (allow_first_axis && ndim == 3 && i == 2 && herm_possible()) {
                DimPass t = ps;
                t.want_half = true;
                t.store_lim = (int)(p.dims[2] / 2);
                if (try_first_axis(t, select_half_store(ps, t))) {
                    ps = t;
                    first_axis = true;
                    return Outcome::Selected;
                }
            }
            if (first_axis && i == 1) {  // the middle pass: only the columns the first pass stored
                ps.col_prefix = p.dims[2] / 2 + 1;
                for (int k = 3; k < ndim; ++k) ps.col_prefix *= p.dims[k];
            }
            // the pass over dimension 1 of a plan whose last pass will be a Hermitian twin: a half-store kernel, tuned or
            // runtime specialised, before anything else
            if (i == 1 && !first_axis && herm_possible()) {
                DimPass t = ps;
                t.want_half = true;
                t.store_lim = (int)(p.dims[1] / 2);
                const bool found = select_half_store(ps, t);
                p.hs_selected = found;
                if (found && last_pass_will_be_hermitian()) {
                    ps = t;
                    return Outcome::Selected;
                }
                if (found) free_pass_tables(t);
                p.hs_selected = false;
            }
            if (select_row2d(p, ps)) return Outcome::Selected;  // 16384-point rows: four-step inside one LDS plane, one launch
            // Long rows of a big batched 1-D transform: two column-tile passes (four-step) move the tensor twice
            // at ~4.7 TB/s each (256 MB: 0.22 ms), which beats one workgroup per 128-KiB row (one workgroup per CU,
            // 2 TB/s: 0.26 ms) once the tensor fills the GPU in both passes; 8192-point rows are still faster in
            // one kernel (0.13 ms).  (Config::fourstep_min_n; 0 = never prefer the four-step.)
            if (ndim == 1 && p.in_components == 2 && p.in_dtype == p.out_dtype && cfg.fourstep_min_n > 0 &&
                ps.N >= cfg.fourstep_min_n && p.size_batch() * (double)ps.N * (double)p.out_elem_bytes() >= cfg.fourstep_min_bytes) {
                std::string why4;
                const size_t before = p.passes.size();
                const Outcome r = routed(build_fourstep(p, i, why4) && p.passes.size() == before + 2, "four-step: ", why4);
                if (r != Outcome::None) return r;
                // no two-pass split: drop whatever was appended and fall through to the single-kernel path
                for (size_t k = before; k < p.passes.size(); ++k) free_pass_tables(p.passes[k]);
                p.passes.resize(before);
                if (p.d_scratch) {
                    (void)hipFree(p.d_scratch);
                    p.d_scratch = nullptr;
                    p.scratch_bytes = 0;
                }
            }
#ifdef MIFFT_EXPERIMENTAL
            // lab knob: strided dimensions of at least Config::fs_strided_min_n points try the two-pass four-step before the
            // single column tile (whose tile narrows to 8 / 4 columns = 64- / 32-byte runs beyond ~1300 / 2600 points)
            if (ps.inner != 1 && cfg.fs_strided_min_n > 0 && (long long)ps.N >= cfg.fs_strided_min_n) {
                std::string whyt;
                const Outcome r = routed(build_fourstep_strided(p, i, whyt), strided_prefix, whyt);
                if (r != Outcome::None) return r;
            }
            std::string whys;
            if (select_jit_streaming_rows(p, ps, whys)) return Outcome::Selected;  // streaming hints on runtime-specialised rows (negative result)
            if (select_dpp_rows(p, ps)) return Outcome::Selected;  // wave-shuffle radix 3 for N = 93 (negative result)
#endif
            // last pass of a real-input 2-D .. 4-D plan: a Hermitian twin (half the columns) beats any full column kernel --
            // a tuned twin first, else the runtime-specialised one, and only then the ordinary tables
            if (ps.want_herm && select_herm(ps)) return Outcome::Selected;
            if (select_fast(p, ps)) return Outcome::Selected;
            // no table entry: specialise the tile kernel for this length now (strided dimensions up to 4096 points;
            // longer ones are better off on the transposed route below)
            std::string whyj;
            if ((ps.inner == 1 || ps.N <= 4096) && select_jit(p, ps, whyj)) return Outcome::Selected;
            // long strided dimension without a fused column tile: transposes + the contiguous-row kernel beat the
            // literal-stage column fallback by an order of magnitude (and lift its 10 240-point limit)
            if (ps.inner != 1 && ps.N > 4096) {
                std::string whyt;
                // two column passes through the scratch (four-step) when both factors have fused tiles ...
                Outcome r = routed(build_fourstep_strided(p, i, whyt), strided_prefix, whyt);
                if (r != Outcome::None) return r;
                // ... else the reference's own route: transpose, contiguous-row kernel, transpose back
                r = routed(build_transposed_dim(p, i, ordered[i], processed[i], whyt),
                           "transposed route of dimension " + std::to_string(i) + ": ", whyt);
                if (r != Outcome::None) return r;
            }
        }
        std::string whyg, why4;
        if (select_generic(p, ps, whyg)) return Outcome::Selected;
        // too long for one workgroup's LDS: four-step over two column-tile passes (contiguous dim of a
        // batched 1-D complex transform; the reference has no path at all here off NVIDIA clusters)
        const Outcome r = routed(i == ndim - 1 && build_fourstep(p, i, why4), "four-step: ", why4);
        if (r != Outcome::None) return r;
        status = MIFFT_ERR_TOO_LARGE;
        why = whyg + (why4.empty() ? "" : "; four-step: " + why4);
        return Outcome::Failed;
    }

    // one schedule attempt: the passes in execution order, last dimension first
    int build_once() {
        for (int i = p.ndim - 1; i >= 0; --i) {
            DimPass ps = pass_of(i);
            // the LAST pass of a real-input 2-D .. 4-D plan may exploit the Hermitian symmetry of what it reads (TileCfg::HERM):
            // half the reads and butterflies, every result stored at (k, c) and conjugated at (-k, -c)
            ps.want_herm = cfg.herm != 0 && i == 0 && p.ndim >= 2 && p.ndim <= 4 && p.in_components == 1 &&
                           !(p.flags & MIFFT_FLAG_FAITHFUL_STAGES) && ps.inner < (1ll << 30);
            const Outcome r = select_pass(i, ps);
            if (r == Outcome::Appended) continue;
            if (r == Outcome::Failed) return status;
            if (const int prc = ps.prepare ? ps.prepare() : MIFFT_OK) {
                free_pass_tables(ps);
                return prc;
            }
            const hipError_t e = upload_twiddles(ps);
            p.passes.push_back(ps);  // (before the check: the plan's owner frees what has been uploaded)
            if (e != hipSuccess) return hip_error(e, "twiddle table upload");
        }
        return MIFFT_OK;
    }

    // the half-spectrum schedule needs all three of its kernels
    bool first_axis_complete() const {
        return p.passes.size() == 3 && p.passes[0].hs && p.passes[1].prefix_ok && p.passes[2].herm_d2 > 0 &&
               p.passes[2].herm_dj == (int)p.dims[2];
    }

    // back to the state before build_once()
    void reset() {
        free_plan_device(p);
        p.passes.clear();
        p.scratch_bytes = 0;
        p.alloc_failed = false;
        p.herm_axis = 1;
        p.hs_selected = false;
        herm_known = -1;
        first_axis = false;
    }
};

}  // namespace

int build_general(Plan& p, const std::vector<std::vector<uint32_t>>& ordered,
                  const std::vector<std::vector<uint32_t>>& processed, std::string& why) {
    Scheduler s{p, config(), ordered, processed};
    s.allow_first_axis = s.cfg.herm_first_axis;
    int rc = s.build_once();
    if (rc == MIFFT_OK && s.first_axis && !s.first_axis_complete()) {  // build the plan again without that schedule
        s.reset();
        s.allow_first_axis = false;
        rc = s.build_once();
    }
    why = s.why;
    if (rc) return rc;
    // a half-store pass is only right in front of a Hermitian last pass (both selections are deterministic; the net under them)
    bool any_hs = false;
    for (const DimPass& q : p.passes) any_hs = any_hs || q.hs;
    if (any_hs && !(p.passes.back().herm_d2 > 0))
        return set_error(MIFFT_ERR_HIP, "internal: half-store pass without a Hermitian last pass");
    if (s.cfg.nd_mode & 2) {  // (the cache policy of mifft_api.cpp, set_cache_policy)
        int k = 0;
        for (DimPass& ps : p.passes) {
            const bool in_place = (ps.src_buf < 0 && !ps.first) || (ps.src_buf == 1 && ps.dst_buf == 1);
            if (in_place) ps.reverse = (k++ % 2) == 0;
        }
    }
    return MIFFT_OK;
}

}  // namespace mifft
