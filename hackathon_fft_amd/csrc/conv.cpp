// conv.cpp -- the fused FFT convolution of real rows: the MIFFT_FLAG_STFT plans whose payload starts with MIFFT_CONV_TAG
// (include/mifft.h).
//
// One launch, no scratch, no padded copy and no spectrum in memory: the packed real-row kernel of the FFT length n with
// TileCfg::CONV set (tile_kernel.h).  Its load zero-extends a row of L samples to n, the passes run, one work item per pair of
// bins multiplies the unpacked spectrum by the filter row's and folds the products back in LDS, the same passes run again as
// the inverse, and the store writes the samples o .. o + Lo - 1.  x is (batch, L, 1) real, out (batch, Lo, 1) real.  The
// filter spectra are the caller's device buffer, (D, n / 2 + 1) complex values of the plan's float type: the plan keeps the
// address it was given and nothing else, so the caller may rewrite the contents between execs and must keep the buffer alive.
//
// The 12-word payload is overlap-save on the same tile (TileCfg::OLS): signal rows of T samples, T possibly far beyond n, are
// convolved as F blocks of n samples every S, one launch row each; block f stores the S samples from c on of its circular
// result, every output sample exactly once.  Still one launch and no scratch: a plan exec covers count * F block rows.
//
// The 16-word payload is either of the two with elementwise gates fused into the tile's load and store (TileCfg::GATE):
// y = b . conv(a . x), a of x's shape, b of out's.  The plan knows only WHICH gates there are; the tensors are arguments of
// every exec (mifft_gated_args through mifft_exec_batch: mifft_api.cpp).
//
// The 20-word payload is partitioned overlap-save (TileCfg::PART), for filters longer than half a block: the filter is P
// partitions of Q taps, H holds (D, P, n / 2 + 1) complex values, and every stored block sums the products of P shifted input
// blocks with the P spectra in registers before the one inverse.  Gated or not (word 11); one launch, no scratch.
//
// The filter-gradient payload (MIFFT_CONV_GRAD_TAG, below) carries the forward plan's gates in its word 11: the kernel multiplies
// x by the pregate and gy by the postgate as it loads them, and the exec takes a mifft_conv_grad_gated_args.
//
// Word 10 of the filter-gradient payload is a stage of the fused partitioned filter gradient: 1 / 2 the same tile storing the
// half spectra of its u-blocks / g-blocks instead of summing them (TileCfg::WSPEC), 3 the lag-group correlation over such
// spectra (lag_corr.hip), which has no transform of its own.  0 is the fused gradient above.
//
// The two-signal payload (MIFFT_CONV_PAIR_TAG, at the end) has no filter spectrum at all: the second operand is a tensor of rows
// like x, both are arguments of every exec (mifft_conv_pair_args), and the tile transforms both (TileCfg::PAIR).
//
// Bits 8..15 of the mode word of every form, the filter-gradient payload included, are the STORAGE type of the rows: 0 the
// plan's float type, or MIFFT_F16 / MIFFT_BF16 under an F32 plan (ConvRequest::io, TileCfg::IT): x, the gates and out are then
// 2-byte elements, widened in the tile's load and rounded once in its store; H and the arithmetic stay float.
#include <algorithm>

#include "mifft_config.h"
#include "mifft_internal.h"

namespace mifft {

// ---- the payload TAG_LO | TAG_HI | D | o | Lo | mode | H_LO | H_HI, or, overlap-save, ---------------------------------------
// ---- TAG_LO | TAG_HI | D | c | S | mode | H_LO | H_HI | F | s0 | Lo | 0, or, gated, ------------------------------------------
// ---- the eight words | F (0: single block) | s0 | Lo | gates | 0 | 0 | 0 | 0, or, partitioned, -------------------------------
// ---- the eight words | F | s0 | Lo | gates (0: none) | 0 | 0 | 0 | 0 | Q | P | 0 | 0 -----------------------------------------
bool conv_detect(int ndim, const uint32_t* bases_flat, const int32_t* bases_len) {
    if (ndim != 2 || !bases_flat || !bases_len) return false;
    return (bases_len[0] == 8 || bases_len[0] == 12 || bases_len[0] == 16 || bases_len[0] == 20) && bases_flat[0] == MIFFT_CONV_TAG_LO && bases_flat[1] == MIFFT_CONV_TAG_HI;
}

// what the convolution payloads share: the flag, direction, dtype and component checks and the limits of n
static int conv_header_check(const Plan& p, const char* tag, std::string& why) {
    const FlagRefusal other[] = {{MIFFT_FLAG_STFT_POWER, "MIFFT_FLAG_STFT_POWER: a convolution has no magnitude or power store"},
                 {MIFFT_FLAG_STFT_CENTER_REFLECT, "a centre bit (MIFFT_FLAG_STFT_CENTER_REFLECT): a convolution has no frames"},
                 {MIFFT_FLAG_STFT_CENTER_ZEROS, "a centre bit (MIFFT_FLAG_STFT_CENTER_ZEROS): a convolution has no frames"},
                 {MIFFT_FLAG_STFT_HOP_MASK, "a hop (MIFFT_FLAG_STFT_HOP): a convolution has no frames"},
                 {MIFFT_FLAG_FAITHFUL_STAGES, "MIFFT_FLAG_FAITHFUL_STAGES: the reference has no convolution to be faithful to"},
                 {MIFFT_FLAG_HALF_SPECTRUM, "MIFFT_FLAG_HALF_SPECTRUM: the spectrum of a fused convolution is never stored"},
                 {MIFFT_FLAG_DCT, "MIFFT_FLAG_DCT"},
                 {MIFFT_FLAG_DCT_ND, "MIFFT_FLAG_DCT_ND"},
                 {MIFFT_FLAG_DCT_ORTHO, "MIFFT_FLAG_DCT_ORTHO"},
                 {MIFFT_FLAG_KEEP_MASK, "MIFFT_FLAG_KEEP_DIM: a convolution plan extends dim 0 and transforms dim 1"},
                 {MIFFT_FLAG_ISTFT, "MIFFT_FLAG_ISTFT: the two mode bits exclude each other"}};
    if (const int rc = refuse_flags(p.flags, other, std::string("a convolution payload (") + tag + ") with ", why)) return rc;
    if (p.inverse) {
        why = "a convolution plan runs its own inverse: inverse must be 0";
        return MIFFT_ERR_UNSUPPORTED;
    }
    if (p.in_components != 1) {
        why = "a convolution reads real rows (in_components = 1)";
        return MIFFT_ERR_BAD_COMPONENTS;
    }
    if (p.in_dtype != p.out_dtype) {
        why = "a convolution reads the plan's own float type (in_dtype == out_dtype)";
        return MIFFT_ERR_BAD_DTYPE;
    }
    const int64_t n = p.dims[1];
    if (n % 2 != 0 || n < 8 || n > (1 << 14)) {
        why = "convolution at an FFT length of " + std::to_string(n) +
              ": the limits of the packed rows are an even length from 8 to 16384";
        return MIFFT_ERR_UNSUPPORTED;
    }
    std::string w;
    if (!tile_family_supported(TileFamily::ConvRows, p, n, 1, w)) {
        why = "convolution at an FFT length of " + std::to_string(n) + ": " + w;
        return MIFFT_ERR_UNSUPPORTED;
    }
    return MIFFT_OK;
}

// ---- the rules: one set for both tags ------------------------------------------------------------------------------------------
// the mode word: bit 0 correlate, bits 8..15 the storage type (0, MIFFT_F16 or MIFFT_BF16; F32 plans only)
static int conv_mode_check(const Plan& p, ConvRequest& r, const char* noun, std::string& why) {
    const uint32_t mode = r.mode, io = (mode >> 8) & 0xffu;
    if ((mode & ~0xff01u) || (io != 0 && io != MIFFT_F16 && io != MIFFT_BF16)) {
        why = std::string("the mode word of a ") + noun + " payload has bit 0 (" + (r.grad ? "the forward correlated" : "correlate") +
              ") and, in bits 8..15, a storage type (0, MIFFT_F16 or MIFFT_BF16) alone, not " + std::to_string(mode);
        return MIFFT_ERR_BAD_BASES;
    }
    if (io != 0 && p.out_dtype != MIFFT_F32) {
        why = std::string("the storage type ") + std::to_string(io) + " in the mode word of a " + noun +
              " payload: 16-bit rows are widened to float, so the plan must be MIFFT_F32";
        return MIFFT_ERR_BAD_DTYPE;
    }
    r.io = (int)io;
    r.mode = mode & 1u;
    return MIFFT_OK;
}

// The geometry of a decoded request `r` against the plan's dims {L, n} and batch; `noun` is "convolution" or
// "filter-gradient".  `blocks`: the words gave c, S, F, s0 and the row's Lo (always in a gradient payload); else o and Lo of
// a single block; `part`: the 20-word form (whatever its Q says).  On success r is the plan's request: mode split, and S = 0 where a gradient's one block holds the whole row.
static int conv_geometry_check(const Plan& p, ConvRequest& r, bool blocks, bool part, const char* noun, std::string& why) {
    const int64_t L = p.dims[0], n = p.dims[1];
    const std::string payload = std::string(noun) + " payload";
    const std::string of_blocks = (r.grad ? "a " : "an overlap-save ") + payload;
    // (one block that holds the whole row is CONV's geometry; everything else, a single block of a longer row included, OLS's)
    const bool whole = r.grad && r.F == 1 && r.s0 == 0 && r.S == r.Lo && L <= n;
    if (blocks && !whole && (L < 2 || L > (1ll << 30))) {
        why = "signal rows of T = " + std::to_string(L) + " samples in an overlap-save " + payload + ": 2 <= T <= 2^30";
        return L < 2 ? MIFFT_ERR_BAD_DIM : MIFFT_ERR_TOO_LARGE;
    }
    if (!blocks && L > n) {
        why = "rows of L = " + std::to_string(L) + " samples are longer than the FFT length n = " + std::to_string(n) +
              " (L > n: rfft(x, n) would crop)";
        return MIFFT_ERR_UNSUPPORTED;
    }
    if (blocks) {
        if (r.S < 1 || r.o + r.S > n) {
            why = "the stored part c = " + std::to_string(r.o) + ", S = " + std::to_string(r.S) + " of every block of " + of_blocks +
                  ": S >= 1 and c + S <= n = " + std::to_string(n);
            return MIFFT_ERR_BAD_BASES;
        }
    } else if (r.Lo < 1 || r.o + r.Lo > n) {
        why = "the output window o = " + std::to_string(r.o) + ", Lo = " + std::to_string(r.Lo) + " of a " + payload +
              ": Lo >= 1 and o + Lo <= n = " + std::to_string(n);
        return MIFFT_ERR_BAD_BASES;
    }
    if (r.D < 1) {
        why = "D = 0 filter rows in a " + payload + ": D >= 1";
        return MIFFT_ERR_BAD_BASES;
    }
    if (r.D > (1ll << 30)) {
        why = "D = " + std::to_string(r.D) + " filter rows: at most 2^30";
        return MIFFT_ERR_TOO_LARGE;
    }
    if (p.batch % r.D != 0) {
        why = "batch = " + std::to_string(p.batch) + " rows is not a multiple of D = " + std::to_string(r.D) + " filter rows";
        return MIFFT_ERR_BAD_BATCH;
    }
    if (const int rc = conv_mode_check(p, r, noun, why)) return rc;
    const uint64_t addr = (uint64_t)(uintptr_t)r.h;
    if (!r.grad && addr == 0) {
        why = "the filter spectrum address H of a " + payload + " is null";
        return MIFFT_ERR_BAD_BASES;
    }
    if (!r.grad && addr % (2 * dtype_size(p.out_dtype)) != 0) {
        why = "the filter spectrum address H of a " + payload + " is not aligned to one complex element (" +
              std::to_string(2 * dtype_size(p.out_dtype)) + " bytes)";
        return MIFFT_ERR_BAD_BASES;
    }
    if (!blocks) return MIFFT_OK;
    const std::string row_samples = r.grad ? " samples per row of gy" : " output samples per row";
    if (r.F < 1 || r.Lo < 1 || (r.grad && r.Lo > (1ll << 30))) {
        why = "F = " + std::to_string(r.F) + " blocks and Lo = " + std::to_string(r.Lo) + row_samples + " in " + of_blocks +
              (r.grad ? ": F >= 1 and 1 <= Lo <= 2^30" : ": F >= 1 and Lo >= 1");
        return MIFFT_ERR_BAD_BASES;
    }
    if (r.Lo <= (r.F - 1) * r.S || r.Lo > r.F * r.S) {
        why = "Lo = " + std::to_string(r.Lo) + row_samples + " against F = " + std::to_string(r.F) + " blocks of S = " +
              std::to_string(r.S) + ": (F - 1) S < Lo <= F S (the last block " + (r.grad ? "stored" : "stores") + " at least one sample)";
        return MIFFT_ERR_BAD_BASES;
    }
    // (partitioned: a block without a live partition stores zeros, so this rule does not apply; Lo is bounded instead)
    if (!part && (r.s0 <= -n || r.s0 + (r.F - 1) * r.S >= L)) {
        why = "block start s0 = " + std::to_string(r.s0) + " with F = " + std::to_string(r.F) + " blocks every S = " +
              std::to_string(r.S) + " samples: a block reads no sample of its row (-n < s0 and s0 + (F - 1) S < T = " +
              std::to_string(L) + ")";
        return MIFFT_ERR_BAD_BASES;
    }
    if (part && r.Lo > (1ll << 30)) {
        why = "Lo = " + std::to_string(r.Lo) + " output samples per row in a partitioned " + payload + ": at most 2^30";
        return MIFFT_ERR_BAD_BASES;
    }
    if (whole) r.S = 0;
    return MIFFT_OK;
}

// the partitions of a 20-word payload against its blocks
static int conv_partition_check(const Plan& p, const ConvRequest& r, std::string& why) {
    const int64_t n = p.dims[1];
    if (r.Q < 1 || r.Q > n - 1) {
        why = "Q = " + std::to_string(r.Q) + " taps per partition in a partitioned convolution payload: 1 <= Q <= n - 1 = " +
              std::to_string(n - 1);
        return MIFFT_ERR_BAD_BASES;
    }
    if (r.S > n - r.Q + 1) {
        why = "S = " + std::to_string(r.S) + " samples stored per block against Q = " + std::to_string(r.Q) +
              " taps per partition: S <= n - Q + 1 = " + std::to_string(n - r.Q + 1) + " (the rest wraps around)";
        return MIFFT_ERR_BAD_BASES;
    }
    if (r.parts < 1 || r.parts * r.Q > (1ll << 30)) {
        why = "P = " + std::to_string(r.parts) + " partitions of Q = " + std::to_string(r.Q) +
              " taps in a partitioned convolution payload: P >= 1 and P Q <= 2^30";
        return MIFFT_ERR_BAD_BASES;
    }
    return MIFFT_OK;
}

// ---- the word layouts: the only code that knows which word sits where --------------------------------------------------------------
// the words first .. last - 1 of a payload are reserved, but for `keep` (a bit per word)
static int conv_reserved_check(const uint32_t* w, int first, int last, uint32_t keep, const char* form, std::string& why) {
    for (int i = first; i < last; ++i)
        if (!((keep >> i) & 1u) && w[i] != 0) {
            why = "the reserved word " + std::to_string(i) + " of " + form + " payload must be 0, not " + std::to_string(w[i]);
            return MIFFT_ERR_BAD_BASES;
        }
    return MIFFT_OK;
}

// the user radices of n behind the payload
static int conv_radices(const uint32_t* bases_flat, const int32_t* bases_len, std::vector<uint64_t>& radices, std::string& why) {
    if (bases_len[1] < 0) {
        why = "negative bases_len";
        return MIFFT_ERR_NO_BASES;
    }
    read_radices(bases_flat, bases_len[0], bases_len[1], radices);
    return MIFFT_OK;
}

// MIFFT_CONV_TAG: 8 words D | o | Lo | mode | H behind the tag; 12: D | c | S | mode | H | F | s0 | Lo | 0; 16: the twelve with
// F = 0 for a single block (o and Lo in words 3 and 4, words 9 and 10 zero) and the gates in word 11, then four zeros; 20: the
// sixteen, gates or 0 in word 11, then Q | P | 0 | 0
int conv_check(Plan& p, const uint32_t* bases_flat, const int32_t* bases_len, FramedPayload& pl, std::string& why) {
    if (const int rc = conv_header_check(p, "MIFFT_CONV_TAG", why)) return rc;
    const uint32_t* w = bases_flat;
    const int len = bases_len[0];
    const bool part = len == 20;
    const bool blocks = len == 12 || part || (len == 16 && w[8] != 0);
    ConvRequest r;
    r.D = w[2];
    r.o = w[3];
    r.mode = w[5];
    r.h = (const void*)(uintptr_t)((uint64_t)w[6] | ((uint64_t)w[7] << 32));
    if (blocks) {
        r.S = w[4];
        r.F = w[8];
        r.s0 = (int32_t)w[9];
        r.Lo = w[10];
    } else {
        r.Lo = w[4];
    }
    if (len >= 16) r.gates = w[11];
    if (part) {
        r.Q = w[16];
        r.parts = w[17];
    }
    if (const int rc = conv_geometry_check(p, r, blocks, part, "convolution", why)) return rc;
    if (len == 12)
        if (const int rc = conv_reserved_check(w, 11, 12, 0, "an overlap-save convolution", why)) return rc;
    if (r.gated() || len == 16) {
        if (!blocks && (w[9] != 0 || w[10] != 0)) {
            why = "words 9 and 10 (s0 = " + std::to_string(w[9]) + ", Lo = " + std::to_string(w[10]) +
                  ") of a gated convolution payload with F = 0 (a single block: o and Lo are words 3 and 4) must be 0";
            return MIFFT_ERR_BAD_BASES;
        }
        if (r.gates < 1 || r.gates > 3) {
            why = "the gates word 11 of a gated convolution payload has bit 0 (pregate) and bit 1 (postgate), at least one of them, not " +
                  std::to_string(r.gates);
            return MIFFT_ERR_BAD_BASES;
        }
        if (const int rc = conv_reserved_check(w, 12, 16, 0, "a gated convolution", why)) return rc;
    }
    if (part) {
        if (const int rc = conv_partition_check(p, r, why)) return rc;
        if (const int rc = conv_reserved_check(w, 12, 20, 3u << 16, "a partitioned convolution", why)) return rc;
    }
    if (const int rc = conv_radices(bases_flat, bases_len, pl.radices, why)) return rc;
    p.conv = r;
    return MIFFT_OK;
}

// the one pass: dim 1 (n points) over the rows of the batch; the tables are the half-spectrum row pass's
int build_conv(Plan& p, const std::vector<uint32_t>& ordered, const std::vector<uint32_t>& processed, std::string& why) {
    const int64_t n = p.dims[1];
    // (outer: overlap-save, the block rows of one signal row; else 1)
    DimPass ps = fused_row_pass(1, n, p.conv.F, ordered, processed, /*half_pitch=*/true);
    if (!select_tile_family(TileFamily::ConvRows, p, ps, why)) return MIFFT_ERR_UNSUPPORTED;
    const hipError_t e = upload_packed_tables(p.out_dtype, false, ps);
    return append_pass(p, ps, e, "convolution table upload");
}

// ---- the filter gradient: TAG_LO | TAG_HI | D | c | S | mode | F | s0 | Lo | P | 0 | gates | 0 x 4 (MIFFT_CONV_GRAD_TAG, include/mifft.h) ----
bool conv_grad_detect(int ndim, const uint32_t* bases_flat, const int32_t* bases_len) {
    if (ndim != 2 || !bases_flat || !bases_len) return false;
    return bases_len[0] == 16 && bases_flat[0] == MIFFT_CONV_GRAD_TAG_LO && bases_flat[1] == MIFFT_CONV_GRAD_TAG_HI;
}

// Stage 3 of the fused partitioned filter gradient (word 10 = MIFFT_CONV_GRAD_STAGE_LAGS): the lag-group correlation over stored
// spectra, D | Fu | Pg | mode | F | m0 | F | P behind the tag, a zero, the 3, then zeros (no gates: they went into stage 1's
// loads).  dims = {max(Fu, 2), n}: Fu stored u-frames per row, the first of them frame m0 (signed); F g-blocks per row; Pg lag groups.
static int conv_lag_check(Plan& p, const uint32_t* w, std::string& why) {
    ConvRequest r;
    r.grad = true;
    r.stage = 3;
    r.D = w[2];
    r.u_frames = w[3];
    r.lag_groups = w[4];
    r.mode = w[5];
    r.F = w[6];
    r.u_first = (int32_t)w[7];
    r.Lo = w[8];
    r.P = w[9];
    if (r.mode & ~1u) {
        why = "the mode word of a lag-group payload (stage 3 of MIFFT_CONV_GRAD_TAG) has bit 0 (the forward correlated) alone: the "
              "spectra are of the plan's float type, not " + std::to_string(r.mode);
        return MIFFT_ERR_BAD_BASES;
    }
    if (r.D < 1 || r.D > (1ll << 30) || p.batch % r.D != 0) {
        why = "D = " + std::to_string(r.D) + " channels in a lag-group payload against batch = " + std::to_string(p.batch) +
              " rows: 1 <= D <= 2^30, and the batch a multiple of it";
        return r.D < 1 ? MIFFT_ERR_BAD_BASES : r.D > (1ll << 30) ? MIFFT_ERR_TOO_LARGE : MIFFT_ERR_BAD_BATCH;
    }
    if (r.lag_groups < 1) {
        why = "Pg = 0 lag groups in a lag-group payload: 1 <= Pg <= 32";
        return MIFFT_ERR_BAD_BASES;
    }
    if (r.lag_groups > 32) {
        why = "Pg = " + std::to_string(r.lag_groups) + " lag groups: the lag-group kernel keeps at most 32 accumulators per bin "
              "(a longer filter: the composed per-partition gradient)";
        return MIFFT_ERR_UNSUPPORTED;
    }
    if (r.F < 1 || r.F > (1ll << 30) || r.Lo != r.F) {
        why = "F = " + std::to_string(r.F) + " g-blocks per row in a lag-group payload (word 6, and again word 8 = " +
              std::to_string(r.Lo) + "): 1 <= F <= 2^30";
        return MIFFT_ERR_BAD_BASES;
    }
    if (std::max<int64_t>(r.u_frames, 2) != p.dims[0] || r.u_frames < 1 || r.u_frames > (1ll << 30)) {
        why = "Fu = " + std::to_string(r.u_frames) + " stored u-frames per row in a lag-group payload against dims[0] = " +
              std::to_string(p.dims[0]) + ": dims[0] = max(Fu, 2) (no plan has a dimension of 1), 1 <= Fu <= 2^30";
        return MIFFT_ERR_BAD_BASES;
    }
    if (r.P > 65535 || r.P > p.batch / r.D) {
        why = "P = " + std::to_string(r.P) + " partial sums per channel in a lag-group payload: at most 65535 and at most the " +
              std::to_string(p.batch / r.D) + " batch entries of a channel (0: the library's choice)";
        return MIFFT_ERR_BAD_BASES;
    }
    if (const int rc = conv_reserved_check(w, 10, 16, 1u << 10, "a lag-group", why)) return rc;
    p.conv = r;
    return MIFFT_OK;
}

// MIFFT_CONV_GRAD_TAG: 16 words, D | c | S | mode | F | s0 | Lo | P behind the tag, the stage (0: the fused gradient, what every
// payload had there before there were stages), the gates of the forward plan (0: none, likewise), then four zeros
int conv_grad_check(Plan& p, const uint32_t* bases_flat, const int32_t* bases_len, FramedPayload& pl, std::string& why) {
    if (const int rc = conv_header_check(p, "MIFFT_CONV_GRAD_TAG", why)) return rc;
    const uint32_t* w = bases_flat;
    if (w[10] > MIFFT_CONV_GRAD_STAGE_LAGS) {
        why = "the reserved word 10 of a filter-gradient payload must be 0, not " + std::to_string(w[10]) +
              " (or a stage of the fused partitioned gradient: 1 / 2 the spectra of the u-blocks / g-blocks stored, 3 the "
              "lag-group correlation)";
        return MIFFT_ERR_BAD_BASES;
    }
    if (w[10] == MIFFT_CONV_GRAD_STAGE_LAGS) {
        if (const int rc = conv_lag_check(p, w, why)) return rc;
        return conv_radices(bases_flat, bases_len, pl.radices, why);
    }
    ConvRequest r;
    r.grad = true;
    r.stage = (int)w[10];
    r.D = w[2];
    r.o = w[3];
    r.S = w[4];
    r.mode = w[5];
    r.F = w[6];
    r.s0 = (int32_t)w[7];
    r.Lo = w[8];
    r.P = w[9];
    r.gates = w[11];
    if (const int rc = conv_geometry_check(p, r, true, false, "filter-gradient", why)) return rc;
    const int64_t pairs = p.batch / r.D * r.F;  // (of one channel)
    if (r.P > 65535 || r.P > pairs) {
        why = "P = " + std::to_string(r.P) + " partial sums per channel in a filter-gradient payload: at most 65535 and at most the " +
              std::to_string(pairs) + " (row, block) pairs of a channel (0: the library's choice)";
        return MIFFT_ERR_BAD_BASES;
    }
    if (r.gates > 3) {
        why = "the gates word 11 of a filter-gradient payload has bit 0 (pregate) and bit 1 (postgate) alone (0: ungated), not " +
              std::to_string(r.gates);
        return MIFFT_ERR_BAD_BASES;
    }
    if (r.stage && (r.gates & ~(uint32_t)r.stage)) {  // (stage 1 loads x alone, stage 2 gy alone)
        why = "the gates word 11 of a filter-gradient payload of stage " + std::to_string(r.stage) + " has bit " +
              std::to_string(r.stage - 1) + " alone (the " + (r.stage == 1 ? "pregate: only x is loaded" : "postgate: only gy is loaded") +
              "), not " + std::to_string(r.gates);
        return MIFFT_ERR_BAD_BASES;
    }
    if (const int rc = conv_reserved_check(w, 10, 16, 3u << 10, "a filter-gradient", why)) return rc;
    if (const int rc = conv_radices(bases_flat, bases_len, pl.radices, why)) return rc;
    p.conv = r;
    return MIFFT_OK;
}

// P of a built pass when the payload left it to the library: D P workgroups fill the device (as many as the persistent
// grid of a row pass would have), every slice keeps at least one full step of TILE pairs, at most 65535
static int64_t conv_grad_partials(const Plan& p, const DimPass& ps) {
    const int64_t want = (int64_t)p.num_cus * pass_wg_per_cu(ps), pairs = p.batch / p.conv.D * p.conv.F;
    const int64_t P = (want + p.conv.D - 1) / p.conv.D;
    return std::max<int64_t>(1, std::min<int64_t>({P, pairs / ps.tile, (int64_t)65535}));
}

// the one pass, as build_conv's; then P.  Stage 3 has no transform: its pass is the precompiled lag-group kernel (lag_corr.hip)
int build_conv_grad(Plan& p, const std::vector<uint32_t>& ordered, const std::vector<uint32_t>& processed, std::string& why) {
    if (p.conv.stage == 3) {
        DimPass ps;
        ps.dim_index = 1;
        ps.N = p.dims[1];
        ps.first = true;
        ps.half_pitch = p.dims[1] / 2 + 1;
        ps.kernel_name = lag_corr_kernel_name(p.out_dtype, (int)p.conv.lag_groups);
        ps.threads = kLagCorrThreads;
        p.passes.push_back(ps);
        if (p.conv.P == 0) p.conv.P = lag_corr_partials(p);
        return MIFFT_OK;
    }
    const int rc = build_conv(p, ordered, processed, why);
    if (rc) return rc;
    if (p.conv.P == 0) p.conv.P = conv_grad_partials(p, p.passes[0]);
    return MIFFT_OK;
}

// ---- two signals: TAG_LO | TAG_HI | K | ea | eb | o | Lo | mode | 0 x 8 (MIFFT_CONV_PAIR_TAG, include/mifft.h) -------------------
bool conv_pair_detect(int ndim, const uint32_t* bases_flat, const int32_t* bases_len) {
    if (ndim != 2 || !bases_flat || !bases_len) return false;
    return bases_len[0] == 16 && bases_flat[0] == MIFFT_CONV_PAIR_TAG_LO && bases_flat[1] == MIFFT_CONV_PAIR_TAG_HI;
}

// dims = {L, n}: x (batch, L, 1), v (batch, K, 1) -> out (batch, Lo, 1).  The pass is build_conv's.
int conv_pair_check(Plan& p, const uint32_t* bases_flat, const int32_t* bases_len, FramedPayload& pl, std::string& why) {
    if (const int rc = conv_header_check(p, "MIFFT_CONV_PAIR_TAG", why)) return rc;
    const uint32_t* w = bases_flat;
    const int64_t L = p.dims[0], n = p.dims[1];
    ConvRequest r;
    r.pair = true;
    r.D = 1;
    r.K = w[2];
    r.ea = w[3];
    r.eb = w[4];
    r.o = w[5];
    r.Lo = w[6];
    r.mode = w[7];
    if (r.K < 1 || r.Lo < 1) {
        why = "K = " + std::to_string(r.K) + " samples per row of v and Lo = " + std::to_string(r.Lo) +
              " output samples per row in a two-signal convolution payload: K >= 1 and Lo >= 1";
        return MIFFT_ERR_BAD_BASES;
    }
    if (r.ea + L > n) {
        why = "rows of L = " + std::to_string(L) + " samples embedded at ea = " + std::to_string(r.ea) +
              " in a two-signal convolution payload: ea + L <= n = " + std::to_string(n);
        return MIFFT_ERR_BAD_BASES;
    }
    if (r.eb + r.K > n) {
        why = "rows of K = " + std::to_string(r.K) + " samples of v embedded at eb = " + std::to_string(r.eb) +
              " in a two-signal convolution payload: eb + K <= n = " + std::to_string(n);
        return MIFFT_ERR_BAD_BASES;
    }
    if (r.o + r.Lo > n) {
        why = "the output window o = " + std::to_string(r.o) + ", Lo = " + std::to_string(r.Lo) +
              " of a two-signal convolution payload: Lo >= 1 and o + Lo <= n = " + std::to_string(n);
        return MIFFT_ERR_BAD_BASES;
    }
    if (r.mode & ~1u) {  // (no storage type: the rows are the plan's own float type)
        why = "the mode word of a two-signal convolution payload has bit 0 (correlate) alone, not " + std::to_string(r.mode);
        return MIFFT_ERR_BAD_BASES;
    }
    if (const int rc = conv_reserved_check(w, 8, 16, 0, "a two-signal convolution", why)) return rc;
    if (const int rc = conv_radices(bases_flat, bases_len, pl.radices, why)) return rc;
    p.conv = r;
    return MIFFT_OK;
}

}  // namespace mifft
