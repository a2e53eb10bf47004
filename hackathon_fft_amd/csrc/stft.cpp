// stft.cpp -- the plans with MIFFT_FLAG_STFT (torch.stft of real signals, the frames leading; include/mifft.h).
//
// One launch, no scratch, no padded copy and no tensor of frames: the packed real-row kernel of the frame length with
// TileCfg::STFT set, whose load takes row r from frame r % F of batch entry r / F of the signal, reflected or zero-extended at
// the ends of a centred plan, and multiplies it by the window (tile_kernel.h).  x is (batch, T, 1) real, out
// (batch, F, n / 2 + 1, 2); the window travels through `bases` as host data and lives in the plan as a device table of the
// plan's float type.
//
// With MIFFT_FLAG_STFT_POWER the same launch stores |X| or |X|^2 as reals (TileCfg::SPEC), (batch, F, n / 2 + 1, 1), or the
// product of that with a filterbank (TileCfg::FB), (batch, F, M, 1): `bases` then carries the window, the power and the
// (n / 2 + 1, M) matrix, which is banded here -- per column the span from its first to its last non-zero row -- and lives in
// the plan as one device table.
//
// A payload tagged with MIFFT_STFT_EXT_TAG adds a log stage (TileCfg::LOG) and a dense (M, Q) matrix after the bands
// (TileCfg::POST) to the same launch: out is then (batch, F, Q, 1), and the matrix follows the band weights in that table.
#include <cmath>
#include <cstring>

#include "mifft_config.h"
#include "mifft_internal.h"

namespace mifft {

// the STFT bits of a plan with neither mode bit (MIFFT_FLAG_STFT, MIFFT_FLAG_ISTFT)
int stft_flag_check(uint32_t flags, std::string& why) {
    if ((flags & MIFFT_FLAG_STFT_POWER) && !(flags & MIFFT_FLAG_STFT)) {
        why = (flags & MIFFT_FLAG_ISTFT) ? "MIFFT_FLAG_STFT_POWER with MIFFT_FLAG_ISTFT: a magnitude or power spectrogram has no inverse"
                                         : "MIFFT_FLAG_STFT_POWER without MIFFT_FLAG_STFT";
        return MIFFT_ERR_UNSUPPORTED;
    }
    if (flags & (MIFFT_FLAG_STFT | MIFFT_FLAG_ISTFT)) return MIFFT_OK;
    if (flags & MIFFT_FLAG_STFT_HOP_MASK) {
        why = "a hop (MIFFT_FLAG_STFT_HOP) without MIFFT_FLAG_STFT";
        return MIFFT_ERR_UNSUPPORTED;
    }
    if (flags & (MIFFT_FLAG_STFT_CENTER_REFLECT | MIFFT_FLAG_STFT_CENTER_ZEROS)) {
        why = "a centre bit (MIFFT_FLAG_STFT_CENTER_REFLECT / MIFFT_FLAG_STFT_CENTER_ZEROS) without MIFFT_FLAG_STFT";
        return MIFFT_ERR_UNSUPPORTED;
    }
    return MIFFT_OK;
}

// checks that need no device: MIFFT_OK, or the status and its reason
int stft_check(const Plan& p, std::string& why) {
    const FlagRefusal other[] = {{MIFFT_FLAG_FAITHFUL_STAGES, "MIFFT_FLAG_FAITHFUL_STAGES: the reference has no STFT to be faithful to"},
                 {MIFFT_FLAG_HALF_SPECTRUM, "MIFFT_FLAG_HALF_SPECTRUM: an STFT plan stores the half spectrum of every frame anyway"},
                 {MIFFT_FLAG_DCT, "MIFFT_FLAG_DCT"},
                 {MIFFT_FLAG_DCT_ND, "MIFFT_FLAG_DCT_ND"},
                 {MIFFT_FLAG_DCT_ORTHO, "MIFFT_FLAG_DCT_ORTHO"},
                 {MIFFT_FLAG_KEEP_MASK, "MIFFT_FLAG_KEEP_DIM: an STFT plan frames dim 0 and transforms dim 1"},
                 {MIFFT_FLAG_ISTFT, "MIFFT_FLAG_ISTFT: the two mode bits exclude each other"}};
    if (const int rc = refuse_flags(p.flags, other, "MIFFT_FLAG_STFT with ", why)) return rc;
    if (p.stft_hop() == 0) {
        why = "MIFFT_FLAG_STFT with hop 0: MIFFT_FLAG_STFT_HOP(h) carries the hop, 1 .. 65535";
        return MIFFT_ERR_UNSUPPORTED;
    }
    if ((p.flags & MIFFT_FLAG_STFT_CENTER_REFLECT) && (p.flags & MIFFT_FLAG_STFT_CENTER_ZEROS)) {
        why = "both centre bits: MIFFT_FLAG_STFT_CENTER_REFLECT and MIFFT_FLAG_STFT_CENTER_ZEROS exclude each other";
        return MIFFT_ERR_UNSUPPORTED;
    }
    if (p.ndim != 2) {
        why = "MIFFT_FLAG_STFT frames the signals of a (batch, T, 1) tensor: ndim must be 2 (dims = {T, n}), not " +
              std::to_string(p.ndim);
        return MIFFT_ERR_UNSUPPORTED;
    }
    if (p.inverse) {
        why = "the inverse STFT is not routed";
        return MIFFT_ERR_UNSUPPORTED;
    }
    if (p.in_components != 1) {
        why = "an STFT reads real signals (in_components = 1)";
        return MIFFT_ERR_BAD_COMPONENTS;
    }
    if (p.in_dtype != p.out_dtype) {
        why = "an STFT reads the plan's own float type (in_dtype == out_dtype)";
        return MIFFT_ERR_BAD_DTYPE;
    }
    const int64_t T = p.dims[0], n = p.dims[1];
    if (T >= (1ll << 31)) {
        why = "signals of 2^31 samples or more (" + std::to_string(T) + "): the frames are addressed in 32 bits";
        return MIFFT_ERR_TOO_LARGE;
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
    if (!tile_family_supported(TileFamily::StftRows, p, n, 1, w)) {
        why = "STFT with frames of " + std::to_string(n) + " points: " + w;
        return MIFFT_ERR_UNSUPPORTED;
    }
    if (!p.stft_center() && T < n) {
        why = "signals of " + std::to_string(T) + " samples are shorter than one frame of " + std::to_string(n) +
              " (T < n without a centre bit)";
        return MIFFT_ERR_UNSUPPORTED;
    }
    if (p.stft_center() == 1 && n / 2 > T - 1) {
        why = "MIFFT_FLAG_STFT_CENTER_REFLECT needs n / 2 <= T - 1 (one reflection): n = " + std::to_string(n) +
              ", T = " + std::to_string(T);
        return MIFFT_ERR_UNSUPPORTED;
    }
    if (p.stft_frames() >= (1ll << 31) - 64) {  // (hop 1 on a signal just below 2^31 samples)
        why = "2^31 frames per signal or more: the frames are counted in 32 bits";
        return MIFFT_ERR_TOO_LARGE;
    }
    return MIFFT_OK;
}

int read_window(const uint32_t* bases_flat, int64_t n, std::vector<double>& window, std::string& why) {
    window.resize((size_t)n);
    for (int64_t j = 0; j < n; ++j) {
        window[(size_t)j] = word_pair(bases_flat + 2 * j);
        if (!std::isfinite(window[(size_t)j])) {
            why = "window value " + std::to_string(j) + " is not finite";
            return MIFFT_ERR_BAD_BASES;
        }
    }
    return MIFFT_OK;
}

void read_radices(const uint32_t* bases_flat, int64_t off, int count, std::vector<uint64_t>& radices) {
    radices.clear();
    for (int k = 0; k < count; ++k) radices.push_back(bases_flat[off + k]);
}

// a header value of the tagged payload that has to be a non-negative integer
static bool header_count(double v, const char* field, int64_t& out, std::string& why) {
    if (!std::isfinite(v) || v < 0 || v != std::floor(v) || v > 9007199254740992.0) {
        why = std::string("the header value ") + field + " of a tagged MIFFT_FLAG_STFT_POWER payload is a non-negative integer, not " +
              std::to_string(v);
        return false;
    }
    out = (int64_t)v;
    return true;
}

// the tagged payload: w | TAG | power | M | Q | log | add | amin | a | c | fb (K, M) | post (M, Q).  Everything but the
// window, which the caller reads as it reads that of every payload.
static int stft_unpack_tagged(Plan& p, const uint32_t* bases_flat, int64_t len0, std::vector<double>& fb, std::vector<double>& post,
                              std::string& why) {
    const int64_t n = p.dims[1], K = n / 2 + 1;
    const bool f64 = p.out_dtype == MIFFT_F64;
    auto bad_len = [&](const std::string& want) {
        why = "bases_len[0] of a tagged MIFFT_FLAG_STFT_POWER payload is " + want + " words (the window, the tag, power, M, Q, log, "
              "add, amin, a, c, an (n / 2 + 1, M) filterbank, an (M, Q) matrix), not " + std::to_string(len0);
        return MIFFT_ERR_BAD_BASES;
    };
    if (len0 < 2 * (n + 9)) return bad_len("2 (n + 9 + K M + M Q) >= " + std::to_string(2 * (n + 9)));
    const uint32_t* hd = bases_flat + 2 * n + 2;  // power, M, Q, log, add, amin, a, c
    const double power = word_pair(hd);
    int64_t M = 0, Q = 0, lg = 0;
    if (!header_count(word_pair(hd + 2), "M", M, why) || !header_count(word_pair(hd + 4), "Q", Q, why) ||
        !header_count(word_pair(hd + 6), "log", lg, why))
        return MIFFT_ERR_BAD_BASES;
    if (!(power == 1.0 || power == 2.0)) {
        why = "the power of a plan with MIFFT_FLAG_STFT_POWER is 1 (magnitude) or 2 (power), not " + std::to_string(power);
        return MIFFT_ERR_BAD_BASES;
    }
    if (lg > 1) {
        why = "the header value log of a tagged MIFFT_FLAG_STFT_POWER payload is 0 or 1, not " + std::to_string(lg);
        return MIFFT_ERR_BAD_BASES;
    }
    if (M > MIFFT_STFT_MAX_BANDS || Q > MIFFT_STFT_MAX_BANDS) {
        why = std::string(M > MIFFT_STFT_MAX_BANDS ? "a filterbank of M = " : "a matrix post of Q = ") +
              std::to_string(M > MIFFT_STFT_MAX_BANDS ? M : Q) + (M > MIFFT_STFT_MAX_BANDS ? " bands" : " columns") +
              ": at most MIFFT_STFT_MAX_BANDS = " + std::to_string(MIFFT_STFT_MAX_BANDS);
        return MIFFT_ERR_TOO_LARGE;
    }
    if (len0 != 2 * (n + 9 + K * M + M * Q))
        return bad_len("2 (n + 9 + K M + M Q) = " + std::to_string(2 * (n + 9 + K * M + M * Q)) + " (M = " + std::to_string(M) +
                       ", Q = " + std::to_string(Q) + ")");
    if (lg) {
        const double add = word_pair(hd + 8), amin = word_pair(hd + 10), a = word_pair(hd + 12), c = word_pair(hd + 14);
        auto round_t = [&](double v) { return f64 ? v : (double)(float)v; };
        if (!std::isfinite(add) || add < 0) {
            why = "add of the log stage is finite and not negative, not " + std::to_string(add);
            return MIFFT_ERR_BAD_BASES;
        }
        if (!(amin > 0) || !(f64 ? std::isnormal(amin) : std::isnormal((float)amin))) {
            why = "amin of the log stage is positive and rounds to a normal number of the plan's float type, not " +
                  std::to_string(amin);
            return MIFFT_ERR_BAD_BASES;
        }
        if (!std::isfinite(a) || a == 0) {
            why = "a of the log stage is finite and not zero, not " + std::to_string(a);
            return MIFFT_ERR_BAD_BASES;
        }
        if (!std::isfinite(c)) {
            why = "c of the log stage is finite, not " + std::to_string(c);
            return MIFFT_ERR_BAD_BASES;
        }
        p.spec_add = round_t(add);
        p.spec_amin = round_t(amin);
        p.spec_a = round_t(a);
        p.spec_c = round_t(c);
        if (!std::isfinite(p.spec_add) || !std::isfinite(p.spec_a) || p.spec_a == 0 || !std::isfinite(p.spec_c)) {
            why = "add, a and c of the log stage stay finite, and a non-zero, when rounded to the plan's float type";
            return MIFFT_ERR_BAD_BASES;
        }
    }
    if (Q > 0 && M == 0) {
        why = "Q = " + std::to_string(Q) + " with M = 0: the matrix post applies to the bands of a filterbank";
        return MIFFT_ERR_UNSUPPORTED;
    }
    if (Q > 0 && M > n / 2 - 1) {
        why = "Q > 0 with M = " + std::to_string(M) + " bands on frames of " + std::to_string(n) +
              " points: the bands of a frame wait in the free halves of its LDS row, M <= n / 2 - 1 = " + std::to_string(n / 2 - 1);
        return MIFFT_ERR_UNSUPPORTED;
    }
    const uint32_t* body = hd + 16;
    fb.resize((size_t)(K * M));
    for (size_t i = 0; i < fb.size(); ++i) {
        fb[i] = word_pair(body + 2 * i);
        if (!std::isfinite(fb[i])) {
            why = "filterbank weight (" + std::to_string(i / (size_t)M) + ", " + std::to_string(i % (size_t)M) + ") is not finite";
            return MIFFT_ERR_BAD_BASES;
        }
    }
    body += 2 * fb.size();
    post.resize((size_t)(M * Q));
    for (size_t i = 0; i < post.size(); ++i) {
        post[i] = word_pair(body + 2 * i);
        if (!std::isfinite(post[i])) {
            why = "post weight (" + std::to_string(i / (size_t)Q) + ", " + std::to_string(i % (size_t)Q) + ") is not finite";
            return MIFFT_ERR_BAD_BASES;
        }
    }
    p.spec_power = (int)power;
    p.spec_bands = M;
    p.spec_post = Q;
    p.spec_log = lg != 0;
    return MIFFT_OK;
}

int stft_unpack_bases(Plan& p, const uint32_t* bases_flat, const int32_t* bases_len, FramedPayload& pl, std::string& why) {
    const int64_t n = p.dims[1], K = n / 2 + 1;
    const bool spec = (p.flags & MIFFT_FLAG_STFT_POWER) != 0;
    pl = FramedPayload();
    std::vector<double>& fb = pl.fb;
    p.spec_power = 0;
    p.spec_bands = 0;
    p.spec_post = 0;
    p.spec_log = false;
    p.spec_add = p.spec_amin = p.spec_a = p.spec_c = 0.0;
    // the extension is chosen by one NaN in the power slot; every other payload means what it has always meant
    const bool tagged = spec && bases_flat && bases_len && (int64_t)bases_len[0] >= 2 * n + 2 &&
                        bases_flat[2 * n] == MIFFT_STFT_EXT_TAG_LO && bases_flat[2 * n + 1] == MIFFT_STFT_EXT_TAG_HI;
    if (tagged) {
        const int rc = stft_unpack_tagged(p, bases_flat, (int64_t)bases_len[0], fb, pl.post, why);
        if (rc) return rc;
    } else if (spec) {  // the window written out, the power, and M columns of K weights: 2 n + 2 + 2 M K words
        const int64_t len0 = bases_len ? (int64_t)bases_len[0] : 0, rest = len0 - 2 * n - 2;
        if (!bases_flat || !bases_len || rest < 0 || rest % (2 * K) != 0) {
            why = "bases_len[0] of a plan with MIFFT_FLAG_STFT_POWER is 2 n + 2 + 2 M K = " + std::to_string(2 * n + 2) + " + " +
                  std::to_string(2 * K) + " M words (the window, the power, an (n / 2 + 1, M) filterbank; M >= 0), not " +
                  (bases_len ? std::to_string(bases_len[0]) : std::string("absent (bases is NULL)"));
            return MIFFT_ERR_BAD_BASES;
        }
        if (rest / (2 * K) > MIFFT_STFT_MAX_BANDS) {
            why = "a filterbank of " + std::to_string(rest / (2 * K)) + " bands: at most MIFFT_STFT_MAX_BANDS = " +
                  std::to_string(MIFFT_STFT_MAX_BANDS);
            return MIFFT_ERR_TOO_LARGE;
        }
        p.spec_bands = rest / (2 * K);
    } else {
        if (!bases_flat || !bases_len) return MIFFT_OK;
        if (bases_len[0] != 0 && (int64_t)bases_len[0] != 2 * n) {
            why = "bases_len[0] of an STFT plan is 0 (rectangular window) or 2 n = " + std::to_string(2 * n) +
                  " words of window, not " + std::to_string(bases_len[0]);
            return MIFFT_ERR_BAD_BASES;
        }
    }
    if (bases_len[1] < 0) {
        why = "negative bases_len";
        return MIFFT_ERR_NO_BASES;
    }
    if (bases_len[0])
        if (const int rc = read_window(bases_flat, n, pl.window, why)) return rc;
    if (spec && !tagged) {
        const double power = word_pair(bases_flat + 2 * n);
        if (!(power == 1.0 || power == 2.0)) {  // (NaN included)
            why = "the power of a plan with MIFFT_FLAG_STFT_POWER is 1 (magnitude) or 2 (power), not " + std::to_string(power);
            return MIFFT_ERR_BAD_BASES;
        }
        p.spec_power = (int)power;
        fb.resize((size_t)(K * p.spec_bands));
        for (size_t i = 0; i < fb.size(); ++i) {
            const double v = word_pair(bases_flat + 2 * n + 2 + 2 * i);
            if (!std::isfinite(v)) {
                why = "filterbank weight (" + std::to_string(i / (size_t)p.spec_bands) + ", " +
                      std::to_string(i % (size_t)p.spec_bands) + ") is not finite";
                return MIFFT_ERR_BAD_BASES;
            }
            fb[i] = v;
        }
    }
    read_radices(bases_flat, bases_len[0], bases_len[1], pl.radices);
    return MIFFT_OK;
}

// the window in the plan's float type: n values, read by the kernel as n / 2 packed pairs
template <typename T>
static hipError_t upload_window_t(int64_t n, const std::vector<double>& window, void** d_table) {
    std::vector<T> tab((size_t)n, (T)1);
    for (size_t j = 0; j < window.size(); ++j) tab[j] = (T)window[j];
    hipError_t e = hipMalloc(d_table, tab.size() * sizeof(T));
    if (e == hipSuccess) e = hipMemcpy(*d_table, tab.data(), tab.size() * sizeof(T), hipMemcpyHostToDevice);
    return e;
}

// ---- MDCT plans: the payload w[0 .. 2M-1] | MIFFT_MDCT_TAG | scale ------------------------------------------------------------
bool mdct_detect(int ndim, const int64_t* dims, const uint32_t* bases_flat, const int32_t* bases_len) {
    if (ndim != 2 || !dims || !bases_flat || !bases_len || dims[1] < 2 || dims[1] > (1 << 20)) return false;
    const int64_t n = dims[1];
    return (int64_t)bases_len[0] == 2 * n + 4 && bases_flat[2 * n] == MIFFT_MDCT_TAG_LO && bases_flat[2 * n + 1] == MIFFT_MDCT_TAG_HI;
}

int mdct_check(Plan& p, const uint32_t* bases_flat, const int32_t* bases_len, FramedPayload& pl, std::string& why) {
    const FlagRefusal other[] = {{MIFFT_FLAG_STFT_POWER, "MIFFT_FLAG_STFT_POWER: an MDCT has no magnitude or power store"},
                 {MIFFT_FLAG_STFT_CENTER_REFLECT, "MIFFT_FLAG_STFT_CENTER_REFLECT: the frames of an MDCT see zeros beyond both ends"},
                 {MIFFT_FLAG_FAITHFUL_STAGES, "MIFFT_FLAG_FAITHFUL_STAGES: the reference has no MDCT to be faithful to"},
                 {MIFFT_FLAG_HALF_SPECTRUM, "MIFFT_FLAG_HALF_SPECTRUM: an MDCT has no half spectrum"},
                 {MIFFT_FLAG_DCT, "MIFFT_FLAG_DCT"},
                 {MIFFT_FLAG_DCT_ND, "MIFFT_FLAG_DCT_ND"},
                 {MIFFT_FLAG_DCT_ORTHO, "MIFFT_FLAG_DCT_ORTHO: the norm of an MDCT travels as the scale of its payload"},
                 {MIFFT_FLAG_KEEP_MASK, "MIFFT_FLAG_KEEP_DIM: an MDCT plan frames dim 0 and transforms dim 1"},
                 {MIFFT_FLAG_ISTFT, "MIFFT_FLAG_ISTFT: the two mode bits exclude each other"}};
    if (const int rc = refuse_flags(p.flags, other, "an MDCT payload (MIFFT_MDCT_TAG) with ", why)) return rc;
    if (!(p.flags & MIFFT_FLAG_STFT_CENTER_ZEROS)) {
        why = "an MDCT payload (MIFFT_MDCT_TAG) without a centre bit: MIFFT_FLAG_STFT_CENTER_ZEROS is required";
        return MIFFT_ERR_UNSUPPORTED;
    }
    const int64_t T = p.dims[0], n = p.dims[1], M = n / 2;
    if (n % 2 != 0) {
        why = "an MDCT frame has 2 M samples: dims[1] = " + std::to_string(n) + " is odd";
        return MIFFT_ERR_UNSUPPORTED;
    }
    if (p.stft_hop() != M) {
        why = "the hop of an MDCT plan is M = dims[1] / 2 = " + std::to_string(M) + " (MIFFT_FLAG_STFT_HOP), not " +
              std::to_string(p.stft_hop());
        return MIFFT_ERR_UNSUPPORTED;
    }
    if (p.inverse) {
        why = "the inverse MDCT is not routed through MIFFT_FLAG_STFT (inverse must be 0): it is the same tag on a MIFFT_FLAG_ISTFT plan";
        return MIFFT_ERR_UNSUPPORTED;
    }
    if (p.in_components != 1) {
        why = "an MDCT reads real signals (in_components = 1)";
        return MIFFT_ERR_BAD_COMPONENTS;
    }
    if (p.in_dtype != p.out_dtype) {
        why = "an MDCT reads the plan's own float type (in_dtype == out_dtype)";
        return MIFFT_ERR_BAD_DTYPE;
    }
    if (T >= (1ll << 31)) {
        why = "signals of 2^31 samples or more (" + std::to_string(T) + "): the frames are addressed in 32 bits";
        return MIFFT_ERR_TOO_LARGE;
    }
    if (M % 2 != 0 || M < 8) {
        why = "MDCT with M = " + std::to_string(M) + " coefficients per frame: M is even and at least 8 (the limits of a DCT-IV row)";
        return MIFFT_ERR_UNSUPPORTED;
    }
    std::string w;
    if (!tile_family_supported(TileFamily::MdctRows, p, M, 1, w)) {
        why = "MDCT with M = " + std::to_string(M) + " coefficients per frame: " + w;
        return MIFFT_ERR_UNSUPPORTED;
    }
    if (bases_len[1] < 0) {
        why = "negative bases_len";
        return MIFFT_ERR_NO_BASES;
    }
    if (const int rc = read_window(bases_flat, n, pl.window, why)) return rc;
    const double scale = word_pair(bases_flat + 2 * n + 2);
    if (!std::isfinite(scale) || scale == 0.0) {
        why = "the scale of an MDCT payload is finite and not zero, not " + std::to_string(scale);
        return MIFFT_ERR_BAD_BASES;
    }
    read_radices(bases_flat, bases_len[0], bases_len[1], pl.radices);
    p.mdct = M;
    p.mdct_scale = scale;
    return MIFFT_OK;
}

// the one pass: a DCT-IV of M points (dim 1) over the F frames of every batch entry, framed, windowed and folded by its load
int build_mdct(Plan& p, const std::vector<uint32_t>& ordered, const std::vector<uint32_t>& processed, const FramedPayload& pl,
               std::string& why) {
    const int64_t M = p.mdct;
    DimPass ps = fused_row_pass(1, M, p.stft_frames(), ordered, processed, /*half_pitch=*/false);
    if (!select_tile_family(TileFamily::MdctRows, p, ps, why)) return MIFFT_ERR_UNSUPPORTED;
    ps.dct_s0 = ps.dct_s1 = p.mdct_scale;  // (X = DCT-IV(u) / 2: the factor 2 of the DCT-IV store is simply not applied)
    hipError_t e = upload_twiddle_table(p.out_dtype, M / 2, false, &ps.d_twiddle);
    if (e == hipSuccess) e = upload_dct4_table(p.out_dtype, M, &ps.d_aux2);
    if (e == hipSuccess)
        e = p.out_dtype == MIFFT_F64 ? upload_window_t<double>(2 * M, pl.window, &ps.d_aux3) : upload_window_t<float>(2 * M, pl.window, &ps.d_aux3);
    return append_pass(p, ps, e, "MDCT table upload");
}

// the (K, M) filterbank as bands: per column lo = its first non-zero row and len = its last non-zero row - lo + 1 (zeros in
// between stay inside the span; a column of zeros has len 0), off = where its len weights start.  One device table: lo[M],
// len[M], off[M] (int32, padded to an even count), then the weights, rounded once to T.
template <typename T>
static hipError_t upload_bands_t(int64_t K, int64_t M, const std::vector<double>& fb, const std::vector<double>& post,
                                 int64_t& post_off, void** d_table) {
    std::vector<int32_t> head((size_t)spec_table_ints(M), 0);
    std::vector<T> wt;
    for (int64_t m = 0; m < M; ++m) {
        int64_t lo = 0, hi = -1;
        for (int64_t k = 0; k < K; ++k)
            if (fb[(size_t)(k * M + m)] != 0.0) {
                if (hi < 0) lo = k;
                hi = k;
            }
        const int64_t len = hi < 0 ? 0 : hi - lo + 1;
        head[(size_t)m] = (int32_t)lo;
        head[(size_t)(M + m)] = (int32_t)len;
        head[(size_t)(2 * M + m)] = (int32_t)wt.size();  // (<= M K < 2^30: bases_len is an int32 of 2 M K words and more)
        for (int64_t j = 0; j < len; ++j) wt.push_back((T)fb[(size_t)((lo + j) * M + m)]);
    }
    post_off = (int64_t)wt.size();  // the dense (M, Q) matrix of a POST configuration, behind the band weights
    for (double v : post) wt.push_back((T)v);
    const size_t hb = head.size() * sizeof(int32_t), wb = wt.size() * sizeof(T);
    hipError_t e = hipMalloc(d_table, hb + (wb ? wb : sizeof(T)));
    if (e == hipSuccess) e = hipMemcpy(*d_table, head.data(), hb, hipMemcpyHostToDevice);
    if (e == hipSuccess && wb) e = hipMemcpy((char*)*d_table + hb, wt.data(), wb, hipMemcpyHostToDevice);
    return e;
}

// the one pass: dim 1 (n points) over the F frames of every batch entry
int build_stft(Plan& p, const std::vector<uint32_t>& ordered, const std::vector<uint32_t>& processed, const FramedPayload& pl,
               std::string& why) {
    const int64_t n = p.dims[1];
    DimPass ps = fused_row_pass(1, n, p.stft_frames(), ordered, processed, /*half_pitch=*/true);
    if (!select_tile_family(TileFamily::StftRows, p, ps, why)) return MIFFT_ERR_UNSUPPORTED;
    hipError_t e = upload_packed_tables(p.out_dtype, false, ps);  // (as a half-spectrum row pass); then the window
    if (e == hipSuccess)
        e = p.out_dtype == MIFFT_F64 ? upload_window_t<double>(n, pl.window, &ps.d_aux2) : upload_window_t<float>(n, pl.window, &ps.d_aux2);
    if (e == hipSuccess && p.spec_bands > 0)
        e = p.out_dtype == MIFFT_F64 ? upload_bands_t<double>(n / 2 + 1, p.spec_bands, pl.fb, pl.post, p.spec_post_off, &ps.d_aux3)
                                     : upload_bands_t<float>(n / 2 + 1, p.spec_bands, pl.fb, pl.post, p.spec_post_off, &ps.d_aux3);
    return append_pass(p, ps, e, "STFT table upload");
}

}  // namespace mifft
