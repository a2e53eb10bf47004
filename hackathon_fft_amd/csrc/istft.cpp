// istft.cpp -- the plans with MIFFT_FLAG_ISTFT (torch.istft with real output, the frames leading; include/mifft.h).
//
// One launch, no scratch, no memset and no tensor of frames: the C2R row kernel of the frame length with TileCfg::ISTFT set,
// whose rows are TILE consecutive frames of one batch entry and whose store multiplies by the synthesis window, overlap-adds
// the frames in LDS, carries the unfinished samples to the workgroup's next tile, divides by the window envelope and writes
// every output sample once (tile_kernel.h).  x is (batch, F, n / 2 + 1, 2), out (batch, T, 1) real.  The window and the gain
// travel through `bases` as host data; the plan keeps gain * w[j] / n with the sign of the kernel's conjugation (the 1 / n is
// folded into this table: the pass's own scale is not applied) and 1 / sum w^2 at every padded sample as device tables of its
// float type, both computed in binary64 and rounded once.
//
// The same flag with a window payload tagged MIFFT_MDCT_TAG is the inverse MDCT (imdct_check, build_imdct below).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>

#include "mifft_config.h"
#include "mifft_internal.h"

namespace mifft {

// sum over the frames that cover padded sample u of w[u - f hop]^2, ascending f
static double envelope_at(const std::vector<double>& window, int64_t n, int64_t hop, int64_t F, int64_t u) {
    const int64_t f_hi = std::min<int64_t>(F - 1, u / hop), f_lo = u < n ? 0 : (u - n) / hop + 1;
    double s = 0.0;
    for (int64_t f = f_lo; f <= f_hi; ++f) {
        const double w = window.empty() ? 1.0 : window[(size_t)(u - f * hop)];
        s += w * w;
    }
    return s;
}

// From u = n on and below F hop every padded sample is covered by the same window values as the one a hop before it, summed
// in the same order: the envelope there repeats with period hop.  `middle` says whether u has such a twin a hop before it.
static bool envelope_repeats(int64_t n, int64_t hop, int64_t F, int64_t u) { return u >= n + hop && u < F * hop; }

// the first stored sample u in [c, c + T) whose envelope is below `tiny` in absolute value, or -1: the head, the tail and ONE
// period of the repeating middle are evaluated, O(n^2 / hop) whatever the length
static int64_t envelope_first_below(const std::vector<double>& window, int64_t n, int64_t hop, int64_t F, int64_t c, int64_t T,
                                    double tiny) {
    int64_t first = -1;
    auto visit = [&](int64_t u) {
        if ((first < 0 || u < first) && std::fabs(envelope_at(window, n, hop, F, u)) < tiny) first = u;
    };
    const int64_t lo = c, hi = c + T;                       // [lo, hi)
    const int64_t m0 = std::max(lo, n + hop), m1 = std::min(hi, F * hop);  // the repeating samples among them
    for (int64_t u = lo; u < std::min(hi, n + hop); ++u) visit(u);
    for (int64_t u = std::max(lo, std::max(F * hop, n + hop)); u < hi; ++u) visit(u);
    for (int64_t u = m0; u < std::min(m1, m0 + hop); ++u) visit(u);  // one period stands for all of them
    return first;
}

// checks that need no device: MIFFT_OK, or the status and its reason; the window, the gain and the user radices on the way.
// `adj_mode` null: an inverse STFT plan.  Else an STFT adjoint plan (stft_adj_check), whose mode word it receives: the covered
// length, the envelope's limit and the overlap-add condition do not apply, and the payload is the tagged one.
static int istft_check_impl(const Plan& p, const uint32_t* bases_flat, const int32_t* bases_len, FramedPayload& pl, std::string& why,
                            int* adj_mode) {
    pl = FramedPayload();
    std::vector<double>& window = pl.window;
    double& gain = pl.gain;
    const FlagRefusal other[] = {// (MIFFT_FLAG_STFT beside this bit never gets here: stft_check refuses the pair)
                 {MIFFT_FLAG_FAITHFUL_STAGES, "MIFFT_FLAG_FAITHFUL_STAGES: the reference has no inverse STFT to be faithful to"},
                 {MIFFT_FLAG_HALF_SPECTRUM, "MIFFT_FLAG_HALF_SPECTRUM: an inverse STFT plan reads the half spectrum of every frame anyway"},
                 {MIFFT_FLAG_DCT, "MIFFT_FLAG_DCT"},
                 {MIFFT_FLAG_DCT_ND, "MIFFT_FLAG_DCT_ND"},
                 {MIFFT_FLAG_DCT_ORTHO, "MIFFT_FLAG_DCT_ORTHO"},
                 {MIFFT_FLAG_KEEP_MASK, "MIFFT_FLAG_KEEP_DIM: an inverse STFT plan transforms dim 2 and overlap-adds dim 1"}};
    if (const int rc = refuse_flags(p.flags, other, "MIFFT_FLAG_ISTFT with ", why)) return rc;
    if (!p.inverse) {
        why = "MIFFT_FLAG_ISTFT with inverse = 0: the forward transform is MIFFT_FLAG_STFT";
        return MIFFT_ERR_UNSUPPORTED;
    }
    if (p.ndim != 3) {
        why = "MIFFT_FLAG_ISTFT overlap-adds the frames of a (batch, F, n / 2 + 1, 2) tensor: ndim must be 3 (dims = {T, F, n}), not " +
              std::to_string(p.ndim);
        return MIFFT_ERR_UNSUPPORTED;
    }
    if ((p.flags & MIFFT_FLAG_STFT_CENTER_REFLECT) && (p.flags & MIFFT_FLAG_STFT_CENTER_ZEROS)) {
        why = "both centre bits: MIFFT_FLAG_STFT_CENTER_REFLECT and MIFFT_FLAG_STFT_CENTER_ZEROS exclude each other";
        return MIFFT_ERR_UNSUPPORTED;
    }
    const int64_t T = p.dims[0], F = p.dims[1], n = p.dims[2], hop = p.stft_hop();
    if (hop == 0) {
        why = "MIFFT_FLAG_ISTFT with hop 0: MIFFT_FLAG_STFT_HOP(h) carries the hop, 1 .. n";
        return MIFFT_ERR_UNSUPPORTED;
    }
    if (hop > n) {
        why = "MIFFT_FLAG_ISTFT with hop " + std::to_string(hop) + " > n = " + std::to_string(n) +
              ": gaps between the frames, where the window envelope is zero";
        return MIFFT_ERR_UNSUPPORTED;
    }
    if (p.in_components != 2) {
        why = "an inverse STFT reads complex frames (in_components = 2)";
        return MIFFT_ERR_BAD_COMPONENTS;
    }
    if (p.in_dtype != p.out_dtype) {
        why = "an inverse STFT reads the plan's own float type (in_dtype == out_dtype)";
        return MIFFT_ERR_BAD_DTYPE;
    }
    if (n % 2 != 0) {
        why = "STFT with an odd frame length (" + std::to_string(n) + ") is not supported";
        return MIFFT_ERR_UNSUPPORTED;
    }
    if (n < 8) {
        why = "STFT with frames of fewer than 8 points (" + std::to_string(n) + ") is not supported";
        return MIFFT_ERR_UNSUPPORTED;
    }
    std::string w;
    if (!tile_family_supported(TileFamily::IstftRows, p, n, 1, w)) {
        why = "STFT with frames of " + std::to_string(n) + " points: " + w;
        return MIFFT_ERR_UNSUPPORTED;
    }
    if (F < 1) {
        why = "an inverse STFT needs at least one frame (dims[1] = " + std::to_string(F) + ")";
        return MIFFT_ERR_BAD_DIM;
    }
    if (F > (1ll << 26)) {  // (before L is formed: L = n + hop (F - 1) stays far inside 64 bits)
        why = adj_mode ? "more than 2^26 frames per entry: the frames of an entry are counted in 32 bits"
                       : "more than 2^26 frames per entry: the envelope table has one entry per padded sample";
        return MIFFT_ERR_TOO_LARGE;
    }
    const int64_t L = p.istft_padded_len(), c = p.istft_trim();
    if (adj_mode) {  // dims[0] is the SIGNAL's length: the frames lie inside the padded signal, and nothing else is asked of it
        if (T < 1 || L > T + 2 * c) {
            why = "T = " + std::to_string(T) + " samples" + (c ? " padded by n / 2 on both sides" : "") + ", but the frames cover " +
                  std::to_string(L) + " (n + hop (F - 1)): more than the signal has";
            return MIFFT_ERR_BAD_DIM;
        }
        if ((p.flags & MIFFT_FLAG_STFT_CENTER_REFLECT) && c > T - 1) {
            why = "MIFFT_FLAG_STFT_CENTER_REFLECT with n / 2 = " + std::to_string(c) + " > T - 1 = " + std::to_string(T - 1) +
                  ": the signal is reflected once at each end";
            return MIFFT_ERR_BAD_DIM;
        }
        if (T + n >= (1ll << 31)) {
            why = "signals of " + std::to_string(T) + " samples per entry: the padded samples are addressed in 32 bits";
            return MIFFT_ERR_TOO_LARGE;
        }
        const int64_t l0 = bases_len[0];  // (stft_adj_detect: 2 n + 6, the tag behind the window)
        if (bases_len[1] != 0 || bases_len[2] < 0) {
            why = "bases_len[1] is 0 (dim 1 is overlap-added, not transformed) and bases_len[2] the radices of n";
            return bases_len[2] < 0 ? MIFFT_ERR_NO_BASES : MIFFT_ERR_BAD_BASES;
        }
        if (const int rc = read_window(bases_flat, n, window, why)) return rc;
        gain = word_pair(bases_flat + 2 * n + 2);
        if (!std::isfinite(gain) || gain == 0.0) {
            why = "the gain is finite and not zero, not " + std::to_string(gain);
            return MIFFT_ERR_BAD_BASES;
        }
        const uint32_t mode = bases_flat[2 * n + 4];
        if (mode < 1 || mode > 3) {
            why = "the mode word is 1 (the gradient of X), 2 (of |X|^2) or 3 (of |X|), not " + std::to_string(mode);
            return MIFFT_ERR_BAD_BASES;
        }
        if (bases_flat[2 * n + 5] != 0) {
            why = "the reserved word behind the mode is 0, not " + std::to_string(bases_flat[2 * n + 5]);
            return MIFFT_ERR_BAD_BASES;
        }
        *adj_mode = (int)mode;
        read_radices(bases_flat, l0, bases_len[2], pl.radices);
        return MIFFT_OK;
    }
    if (L > (1ll << 26)) {
        why = "frames that cover " + std::to_string(L) + " samples per entry: the envelope table (one entry per padded sample) is " +
              "limited to 2^26";
        return MIFFT_ERR_TOO_LARGE;
    }
    if (T < 1 || T > L - c) {
        why = "T = " + std::to_string(T) + " output samples, but the frames cover 1 .. " + std::to_string(L - c) +
              " (n + hop (F - 1)" + (c ? " - n / 2" : "") + "): a longer output is not zero-padded";
        return MIFFT_ERR_BAD_DIM;
    }
    // ---- `bases`: window [+ gain], nothing for dim 1, the radices of n ----
    if (bases_flat && bases_len) {
        const int64_t l0 = bases_len[0];
        if (l0 != 0 && l0 != 2 * n && l0 != 2 * n + 2) {
            why = "bases_len[0] of an inverse STFT plan is 0 (rectangular window), 2 n = " + std::to_string(2 * n) +
                  " words of window, or 2 n + 2 (window and gain), not " + std::to_string(l0);
            return MIFFT_ERR_BAD_BASES;
        }
        if (bases_len[1] != 0 || bases_len[2] < 0) {
            why = "bases_len[1] of an inverse STFT plan is 0 (dim 1 is overlap-added, not transformed) and bases_len[2] the radices of n";
            return bases_len[2] < 0 ? MIFFT_ERR_NO_BASES : MIFFT_ERR_BAD_BASES;
        }
        if (l0)
            if (const int rc = read_window(bases_flat, n, window, why)) return rc;
        if (l0 == 2 * n + 2) {
            gain = word_pair(bases_flat + 2 * n);
            if (!std::isfinite(gain)) {
                why = "the gain is not finite";
                return MIFFT_ERR_BAD_BASES;
            }
        }
        read_radices(bases_flat, l0, bases_len[2], pl.radices);
    }
    // ---- NOLA over the samples the plan stores (torch.istft: window_envelop.abs().min() over [c, c + T) against 1e-11) ----
    const int64_t bare = envelope_first_below(window, n, hop, F, c, T, 1e-11);
    if (bare >= 0) {
        why = "the window's squared overlap-add is zero at output sample " + std::to_string(bare - c) +
              " (nonzero overlap-add condition: below 1e-11)";
        return MIFFT_ERR_UNSUPPORTED;
    }
    return MIFFT_OK;
}

int istft_check(const Plan& p, const uint32_t* bases_flat, const int32_t* bases_len, FramedPayload& pl, std::string& why) {
    return istft_check_impl(p, bases_flat, bases_len, pl, why, nullptr);
}

// ---- STFT adjoint plans: the payload w[0 .. n-1] | MIFFT_STFT_ADJ_TAG | gain | mode, 0 on a MIFFT_FLAG_ISTFT plan ------------------
// The gradient of the framed, windowed, one-sided transform with respect to the signal is an overlap-add of inverse real
// transforms: the ISTFT pass with TileCfg::ADJ (tile_kernel.h), no envelope, dims[0] the signal's length.  With g~ the incoming
// gradient whose bins 0 and n / 2 are doubled, frame f contributes w[j] (n / 2) irfft(g~_f)[j]; the pass leaves n irfft(.), so
// the synthesis table is gain * w / 2 -- gain * w for mode 2, whose factor 2 (d|X|^2 = 2 X) lives there.
bool stft_adj_detect(int ndim, const int64_t* dims, const uint32_t* bases_flat, const int32_t* bases_len) {
    if (ndim != 3 || !bases_flat || !bases_len) return false;
    const int64_t n = dims[2];
    return (int64_t)bases_len[0] == 2 * n + 6 && bases_flat[2 * n] == MIFFT_STFT_ADJ_TAG_LO && bases_flat[2 * n + 1] == MIFFT_STFT_ADJ_TAG_HI;
}

int stft_adj_check(Plan& p, const uint32_t* bases_flat, const int32_t* bases_len, FramedPayload& pl, std::string& why) {
    int mode = 0;
    const int rc = istft_check_impl(p, bases_flat, bases_len, pl, why, &mode);
    if (rc) {
        why = "an STFT adjoint payload (MIFFT_STFT_ADJ_TAG on a MIFFT_FLAG_ISTFT plan): " + why;
        return rc;
    }
    p.stft_adj = mode;
    return MIFFT_OK;
}

template <typename T>
static hipError_t upload_t(const std::vector<T>& tab, void** d_table) {
    hipError_t e = hipMalloc(d_table, tab.size() * sizeof(T));
    if (e == hipSuccess) e = hipMemcpy(*d_table, tab.data(), tab.size() * sizeof(T), hipMemcpyHostToDevice);
    return e;
}

// The reciprocal envelope at every padded sample 0 .. n + hop (F - 1) - 1, formed in binary64 and rounded once to the plan's
// type T (the only host copy of the L-entry table is of that type; a repeating sample copies its twin's rounded value, which
// is the same rounding).  The inverse plan and its adjoint both come here, so both divide by the same numbers.
template <typename T>
static std::vector<T> envelope_table_t(int64_t n, int64_t hop, int64_t F, const std::vector<double>& window) {
    const int64_t L = n + hop * (F - 1);
    std::vector<T> inv((size_t)L);
    // (samples outside the stored range may have a zero envelope: their entries are never read)
    for (int64_t u = 0; u < L; ++u) {
        if (envelope_repeats(n, hop, F, u)) {
            inv[(size_t)u] = inv[(size_t)(u - hop)];
            continue;
        }
        const double e = envelope_at(window, n, hop, F, u);
        inv[(size_t)u] = (T)(e != 0.0 ? 1.0 / e : 0.0);
    }
    return inv;
}

// the synthesis table, formed in binary64 and rounded once, and the reciprocal envelope
template <typename T>
static hipError_t upload_tables_t(int64_t n, int64_t hop, int64_t F, const std::vector<double>& window, double gain, void** d_ws,
                                  void** d_env) {
    std::vector<T> ws((size_t)n);
    // the kernel's last pass leaves conj(z) of the packed frame z_m = y[2m] + i y[2m+1], unscaled: odd reals negated, 1 / n here
    for (int64_t j = 0; j < n; ++j)
        ws[(size_t)j] = (T)(((j & 1) ? -gain : gain) * (window.empty() ? 1.0 : window[(size_t)j]) / (double)n);
    hipError_t e = upload_t<T>(ws, d_ws);
    if (e == hipSuccess) e = upload_t<T>(envelope_table_t<T>(n, hop, F, window), d_env);
    return e;
}

// ---- inverse STFT adjoint plans: the payload w[0 .. n-1] | MIFFT_ISTFT_ADJ_TAG | gain | frames, 0 on a MIFFT_FLAG_STFT plan ---------
// The gradient of an inverse STFT plan's result with respect to its frames is the one-sided STFT of gy / envelope: the STFT
// pass with TileCfg::IADJ (tile_kernel.h), whose load multiplies by the inverse plan's reciprocal envelope inside [0, T) and
// selects zeros outside, and whose store halves bins 0 and n / 2.  dims = {T, n}; the frame count F is the payload's -- that of
// X, which `length` may have cropped -- not stft_frames' of T.  The analysis table is 2 gain w / n.
bool istft_adj_detect(int ndim, const int64_t* dims, const uint32_t* bases_flat, const int32_t* bases_len) {
    if (ndim != 2 || !dims || !bases_flat || !bases_len || dims[1] < 2 || dims[1] > (1 << 20)) return false;
    const int64_t n = dims[1];
    return (int64_t)bases_len[0] == 2 * n + 6 && bases_flat[2 * n] == MIFFT_ISTFT_ADJ_TAG_LO && bases_flat[2 * n + 1] == MIFFT_ISTFT_ADJ_TAG_HI;
}

int istft_adj_check(Plan& p, const uint32_t* bases_flat, const int32_t* bases_len, FramedPayload& pl, std::string& why) {
    pl = FramedPayload();
    const char* who = "an inverse STFT adjoint payload (MIFFT_ISTFT_ADJ_TAG)";
    const FlagRefusal other[] = {{MIFFT_FLAG_STFT_POWER, "MIFFT_FLAG_STFT_POWER: the adjoint stores complex bins"},
                 {MIFFT_FLAG_STFT_CENTER_REFLECT, "MIFFT_FLAG_STFT_CENTER_REFLECT: a centred adjoint sees zeros beyond both ends "
                                                  "(MIFFT_FLAG_STFT_CENTER_ZEROS)"},
                 {MIFFT_FLAG_FAITHFUL_STAGES, "MIFFT_FLAG_FAITHFUL_STAGES: the reference has no STFT to be faithful to"},
                 {MIFFT_FLAG_HALF_SPECTRUM, "MIFFT_FLAG_HALF_SPECTRUM: the adjoint stores the half spectrum of every frame anyway"},
                 {MIFFT_FLAG_DCT, "MIFFT_FLAG_DCT"},
                 {MIFFT_FLAG_DCT_ND, "MIFFT_FLAG_DCT_ND"},
                 {MIFFT_FLAG_DCT_ORTHO, "MIFFT_FLAG_DCT_ORTHO"},
                 {MIFFT_FLAG_KEEP_MASK, "MIFFT_FLAG_KEEP_DIM: the adjoint frames dim 0 and transforms dim 1"},
                 {MIFFT_FLAG_ISTFT, "MIFFT_FLAG_ISTFT: the two mode bits exclude each other"}};
    if (const int rc = refuse_flags(p.flags, other, std::string(who) + " with ", why)) return rc;
    const int64_t T = p.dims[0], n = p.dims[1], hop = p.stft_hop();
    if (hop == 0) {
        why = std::string(who) + " with hop 0: MIFFT_FLAG_STFT_HOP(h) carries the hop, 1 .. n";
        return MIFFT_ERR_UNSUPPORTED;
    }
    if (p.inverse) {
        why = std::string(who) + " with inverse = 1: the adjoint of the inverse is a forward plan";
        return MIFFT_ERR_UNSUPPORTED;
    }
    if (p.in_components != 1) {
        why = std::string(who) + " reads real gradients (in_components = 1)";
        return MIFFT_ERR_BAD_COMPONENTS;
    }
    if (p.in_dtype != p.out_dtype) {
        why = std::string(who) + " reads the plan's own float type (in_dtype == out_dtype)";
        return MIFFT_ERR_BAD_DTYPE;
    }
    if (n % 2 != 0) {
        why = "STFT with an odd frame length (" + std::to_string(n) + ") is not supported";
        return MIFFT_ERR_UNSUPPORTED;
    }
    if (n < 8) {
        why = "STFT with frames of fewer than 8 points (" + std::to_string(n) + ") is not supported";
        return MIFFT_ERR_UNSUPPORTED;
    }
    if (bases_len[1] < 0) {
        why = "negative bases_len";
        return MIFFT_ERR_NO_BASES;
    }
    if (const int rc = read_window(bases_flat, n, pl.window, why)) return rc;
    pl.gain = word_pair(bases_flat + 2 * n + 2);
    if (!std::isfinite(pl.gain) || pl.gain == 0.0) {
        why = "the gain of " + std::string(who) + " is finite and not zero, not " + std::to_string(pl.gain);
        return MIFFT_ERR_BAD_BASES;
    }
    const int64_t F = bases_flat[2 * n + 4];
    if (bases_flat[2 * n + 5] != 0) {
        why = "the reserved word behind the frame count of " + std::string(who) + " is 0, not " + std::to_string(bases_flat[2 * n + 5]);
        return MIFFT_ERR_BAD_BASES;
    }
    if (F < 1) {
        why = std::string(who) + " needs at least one frame (the frame count word is 0)";
        return MIFFT_ERR_BAD_DIM;
    }
    // ---- the limits of the inverse plan it is the adjoint of, in that plan's terms ----
    if (hop > n) {
        why = std::string(who) + " with hop " + std::to_string(hop) + " > n = " + std::to_string(n) +
              ": gaps between the frames, where the window envelope is zero";
        return MIFFT_ERR_UNSUPPORTED;
    }
    if (F > (1ll << 26)) {
        why = "more than 2^26 frames per entry: the envelope table has one entry per padded sample";
        return MIFFT_ERR_TOO_LARGE;
    }
    const bool centred = (p.flags & MIFFT_FLAG_STFT_CENTER_ZEROS) != 0;
    const int64_t L = n + hop * (F - 1), c = centred ? n / 2 : 0;
    if (L > (1ll << 26)) {
        why = "frames that cover " + std::to_string(L) + " samples per entry: the envelope table (one entry per padded sample) is " +
              "limited to 2^26";
        return MIFFT_ERR_TOO_LARGE;
    }
    if (T < 1 || T > L - c) {
        why = "T = " + std::to_string(T) + " samples of gradient, but the frames cover 1 .. " + std::to_string(L - c) +
              " (n + hop (F - 1)" + (c ? " - n / 2" : "") + "): the inverse plan stores no more";
        return MIFFT_ERR_BAD_DIM;
    }
    const int64_t bare = envelope_first_below(pl.window, n, hop, F, c, T, 1e-11);
    if (bare >= 0) {
        why = "the window's squared overlap-add is zero at sample " + std::to_string(bare - c) +
              " (nonzero overlap-add condition: below 1e-11)";
        return MIFFT_ERR_UNSUPPORTED;
    }
    std::string w;
    if (!tile_family_supported(TileFamily::StftRows, p, n, 1, w)) {
        why = "STFT with frames of " + std::to_string(n) + " points: " + w;
        return MIFFT_ERR_UNSUPPORTED;
    }
    read_radices(bases_flat, bases_len[0], bases_len[1], pl.radices);
    p.istft_adj = F;
    return MIFFT_OK;
}

template <typename T>
static hipError_t upload_istft_adj_tables_t(int64_t n, int64_t hop, int64_t F, const std::vector<double>& window, double gain,
                                            void** d_win, void** d_env) {
    std::vector<T> wa((size_t)n);  // 2 gain w[j] / n: the store halves bins 0 and n / 2, both factors exact
    for (int64_t j = 0; j < n; ++j) wa[(size_t)j] = (T)(2.0 * gain * window[(size_t)j] / (double)n);
    hipError_t e = upload_t<T>(wa, d_win);
    if (e == hipSuccess) e = upload_t<T>(envelope_table_t<T>(n, hop, F, window), d_env);
    return e;
}

// the one pass: dim 1 (n points) over the payload's F frames of every batch entry
int build_istft_adj(Plan& p, const std::vector<uint32_t>& ordered, const std::vector<uint32_t>& processed, const FramedPayload& pl,
                    std::string& why) {
    const int64_t n = p.dims[1], F = p.istft_adj, hop = p.stft_hop();
    DimPass ps = fused_row_pass(1, n, F, ordered, processed, /*half_pitch=*/true);
    if (!select_tile_family(TileFamily::StftRows, p, ps, why)) return MIFFT_ERR_UNSUPPORTED;
    hipError_t e = upload_packed_tables(p.out_dtype, false, ps);
    if (e == hipSuccess) {
        try {
            e = p.out_dtype == MIFFT_F64 ? upload_istft_adj_tables_t<double>(n, hop, F, pl.window, pl.gain, &ps.d_aux2, &ps.d_aux3)
                                         : upload_istft_adj_tables_t<float>(n, hop, F, pl.window, pl.gain, &ps.d_aux2, &ps.d_aux3);
        } catch (const std::bad_alloc&) {  // (up to 2^26 entries on the host)
            e = hipErrorOutOfMemory;
        }
    }
    return append_pass(p, ps, e, "inverse STFT adjoint table upload");
}

// ---- IMDCT plans: the payload w[0 .. 2M-1] | MIFFT_MDCT_TAG | gain on a MIFFT_FLAG_ISTFT plan -------------------------------------
// One launch, no scratch: the DCT-IV row kernel of M points with TileCfg::IMDCT set, whose store unfolds the M values of a frame
// to its 2 M samples, multiplies by gain * w and adds the two half-frames that meet in every block of M output samples
// (tile_kernel.h).  x is (batch, F, M, 1) real, out (batch, T, 1).  There is no envelope: time-domain aliasing cancellation
// needs none, so there is no overlap-add condition to check either.
bool imdct_detect(int ndim, const uint32_t* bases_flat, const int32_t* bases_len) {
    if (ndim != 3 || !bases_flat || !bases_len || bases_len[0] < 4) return false;
    const int64_t l0 = bases_len[0];
    return bases_flat[l0 - 4] == MIFFT_MDCT_TAG_LO && bases_flat[l0 - 3] == MIFFT_MDCT_TAG_HI;
}

int imdct_check(Plan& p, const uint32_t* bases_flat, const int32_t* bases_len, FramedPayload& pl, std::string& why) {
    pl = FramedPayload();
    const char* who = "an IMDCT payload (MIFFT_MDCT_TAG on a MIFFT_FLAG_ISTFT plan)";
    const FlagRefusal other[] = {{MIFFT_FLAG_STFT_CENTER_REFLECT, "MIFFT_FLAG_STFT_CENTER_REFLECT: the frames of an MDCT see zeros beyond both ends"},
                 {MIFFT_FLAG_FAITHFUL_STAGES, "MIFFT_FLAG_FAITHFUL_STAGES: the reference has no MDCT to be faithful to"},
                 {MIFFT_FLAG_HALF_SPECTRUM, "MIFFT_FLAG_HALF_SPECTRUM: an MDCT has no half spectrum"},
                 {MIFFT_FLAG_DCT, "MIFFT_FLAG_DCT"},
                 {MIFFT_FLAG_DCT_ND, "MIFFT_FLAG_DCT_ND"},
                 {MIFFT_FLAG_DCT_ORTHO, "MIFFT_FLAG_DCT_ORTHO: the norm of an IMDCT travels as the gain of its payload"},
                 {MIFFT_FLAG_KEEP_MASK, "MIFFT_FLAG_KEEP_DIM: an IMDCT plan transforms dim 2 and overlap-adds dim 1"}};
    if (const int rc = refuse_flags(p.flags, other, std::string(who) + " with ", why)) return rc;
    if (!(p.flags & MIFFT_FLAG_STFT_CENTER_ZEROS)) {
        why = std::string(who) + " without a centre bit: MIFFT_FLAG_STFT_CENTER_ZEROS is required";
        return MIFFT_ERR_UNSUPPORTED;
    }
    if (!p.inverse) {
        why = std::string(who) + " with inverse = 0: the forward transform is the tagged MIFFT_FLAG_STFT plan";
        return MIFFT_ERR_UNSUPPORTED;
    }
    const int64_t T = p.dims[0], F = p.dims[1], n = p.dims[2], M = n / 2;
    if (n % 2 != 0) {
        why = "an MDCT frame has 2 M samples: dims[2] = " + std::to_string(n) + " is odd";
        return MIFFT_ERR_UNSUPPORTED;
    }
    if (p.stft_hop() != M) {
        why = "the hop of an IMDCT plan is M = dims[2] / 2 = " + std::to_string(M) + " (MIFFT_FLAG_STFT_HOP), not " +
              std::to_string(p.stft_hop());
        return MIFFT_ERR_UNSUPPORTED;
    }
    if (p.in_components != 1) {
        why = "an IMDCT reads real coefficients (in_components = 1)";
        return MIFFT_ERR_BAD_COMPONENTS;
    }
    if (p.in_dtype != p.out_dtype) {
        why = "an IMDCT reads the plan's own float type (in_dtype == out_dtype)";
        return MIFFT_ERR_BAD_DTYPE;
    }
    if (M % 2 != 0 || M < 8) {
        why = "IMDCT with M = " + std::to_string(M) + " coefficients per frame: M is even and at least 8 (the limits of a DCT-IV row)";
        return MIFFT_ERR_UNSUPPORTED;
    }
    std::string w;
    if (!tile_family_supported(TileFamily::ImdctRows, p, M, 1, w)) {
        why = "IMDCT with M = " + std::to_string(M) + " coefficients per frame: " + w;
        return MIFFT_ERR_UNSUPPORTED;
    }
    if (F < 2) {
        why = "an IMDCT needs at least two frames (dims[1] = " + std::to_string(F) + "): every output sample is the sum of two";
        return MIFFT_ERR_BAD_DIM;
    }
    if (F > (1ll << 26)) {
        why = "more than 2^26 frames per entry (dims[1] = " + std::to_string(F) + ")";
        return MIFFT_ERR_TOO_LARGE;
    }
    if (T < 2 || T > (F - 1) * M) {
        why = "T = dims[0] = " + std::to_string(T) + " output samples, but " + std::to_string(F) + " frames cover 2 .. " +
              std::to_string((F - 1) * M) + " ((F - 1) M): a longer output is not zero-padded";
        return MIFFT_ERR_BAD_DIM;
    }
    if (T >= (1ll << 31)) {
        why = "outputs of 2^31 samples or more per entry (dims[0] = " + std::to_string(T) + "): the samples are addressed in 32 bits";
        return MIFFT_ERR_TOO_LARGE;
    }
    const int64_t l0 = bases_len[0];
    if (l0 != 2 * n + 4) {
        why = "bases_len[0] of an IMDCT plan is exactly 2 (2 M) + 4 = " + std::to_string(2 * n + 4) +
              " words (w[0 .. 2M-1] | TAG | gain), not " + std::to_string(l0);
        return MIFFT_ERR_BAD_BASES;
    }
    if (bases_len[1] != 0 || bases_len[2] < 0) {
        why = "bases_len[1] of an IMDCT plan is 0 (dim 1 is overlap-added, not transformed) and bases_len[2] the radices of M / 2";
        return bases_len[2] < 0 ? MIFFT_ERR_NO_BASES : MIFFT_ERR_BAD_BASES;
    }
    if (const int rc = read_window(bases_flat, n, pl.window, why)) return rc;
    pl.gain = word_pair(bases_flat + 2 * n + 2);
    if (!std::isfinite(pl.gain) || pl.gain == 0.0) {
        why = "the gain of an IMDCT payload is finite and not zero, not " + std::to_string(pl.gain);
        return MIFFT_ERR_BAD_BASES;
    }
    read_radices(bases_flat, l0, bases_len[2], pl.radices);
    p.imdct = M;
    return MIFFT_OK;
}

// the one pass: a DCT-IV of M points (dim 2) over the F frames of every batch entry, unfolded and overlap-added by its store
int build_imdct(Plan& p, const std::vector<uint32_t>& ordered, const std::vector<uint32_t>& processed, const FramedPayload& pl,
                std::string& why) {
    const int64_t M = p.imdct;
    const std::vector<double>& window = pl.window;
    const double gain = pl.gain;
    DimPass ps = fused_row_pass(2, M, p.dims[1], ordered, processed, /*half_pitch=*/false);
    if (!select_tile_family(TileFamily::ImdctRows, p, ps, why)) return MIFFT_ERR_UNSUPPORTED;
    // (the sweep leaves the plain cosine sums: the whole scale is in the table below, and dct_s1 is not applied)
    hipError_t e = upload_twiddle_table(p.out_dtype, M / 2, false, &ps.d_twiddle);
    if (e == hipSuccess) e = upload_dct4_table(p.out_dtype, M, &ps.d_aux2);
    if (e == hipSuccess) {  // ws[j] = gain * w[j], formed in binary64 and rounded once
        if (p.out_dtype == MIFFT_F64) {
            std::vector<double> ws((size_t)(2 * M));
            for (int64_t j = 0; j < 2 * M; ++j) ws[(size_t)j] = gain * window[(size_t)j];
            e = upload_t<double>(ws, &ps.d_aux3);
        } else {
            std::vector<float> ws((size_t)(2 * M));
            for (int64_t j = 0; j < 2 * M; ++j) ws[(size_t)j] = (float)(gain * window[(size_t)j]);
            e = upload_t<float>(ws, &ps.d_aux3);
        }
    }
    return append_pass(p, ps, e, "IMDCT table upload");
}

// the one pass: dim 2 (n points) over the F frames of every batch entry
int build_istft(Plan& p, const std::vector<uint32_t>& ordered, const std::vector<uint32_t>& processed, const FramedPayload& pl,
                std::string& why) {
    const int64_t F = p.dims[1], n = p.dims[2], hop = p.stft_hop();
    const std::vector<double>& window = pl.window;
    const double gain = pl.gain;
    DimPass ps = fused_row_pass(2, n, F, ordered, processed, /*half_pitch=*/true);
    if (!select_tile_family(TileFamily::IstftRows, p, ps, why)) return MIFFT_ERR_UNSUPPORTED;
    hipError_t e = upload_packed_tables(p.out_dtype, true, ps);  // (as an inverse half-spectrum row pass)
    if (e == hipSuccess && p.stft_adj) {  // ws[j] = gain * w[j] / 2 (mode 2: gain * w[j]) with the sign of the conjugation; no envelope
        const double g = p.stft_adj == 2 ? gain : 0.5 * gain;
        std::vector<double> ws((size_t)n);
        for (int64_t j = 0; j < n; ++j) ws[(size_t)j] = ((j & 1) ? -g : g) * (window.empty() ? 1.0 : window[(size_t)j]);
        if (p.out_dtype == MIFFT_F64) {
            e = upload_t<double>(ws, &ps.d_aux2);
        } else {
            e = upload_t<float>(std::vector<float>(ws.begin(), ws.end()), &ps.d_aux2);
        }
    } else if (e == hipSuccess) {
        try {
            e = p.out_dtype == MIFFT_F64 ? upload_tables_t<double>(n, hop, F, window, gain, &ps.d_aux2, &ps.d_aux3)
                                         : upload_tables_t<float>(n, hop, F, window, gain, &ps.d_aux2, &ps.d_aux3);
        } catch (const std::bad_alloc&) {  // (up to 2^26 entries on the host)
            e = hipErrorOutOfMemory;
        }
    }
    return append_pass(p, ps, e, "inverse STFT table upload");
}

}  // namespace mifft
