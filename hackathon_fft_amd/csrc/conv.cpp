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
// Bits 8..15 of the mode word of every form, the filter-gradient payload included, are the STORAGE type of the rows: 0 the
// plan's float type, or MIFFT_F16 / MIFFT_BF16 under an F32 plan (Plan::conv_io, TileCfg::IT): x, the gates and out are then
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
// the mode word of both payloads: bit 0 correlate, bits 8..15 the storage type (0, MIFFT_F16 or MIFFT_BF16; F32 plans only)
static int conv_mode_check(Plan& p, uint32_t mode, const char* what, const char* bit0, std::string& why) {
    const uint32_t io = (mode >> 8) & 0xffu;
    if ((mode & ~0xff01u) || (io != 0 && io != MIFFT_F16 && io != MIFFT_BF16)) {
        why = std::string("the mode word of a ") + what + " payload has bit 0 (" + bit0 +
              ") and, in bits 8..15, a storage type (0, MIFFT_F16 or MIFFT_BF16) alone, not " + std::to_string(mode);
        return MIFFT_ERR_BAD_BASES;
    }
    if (io != 0 && p.out_dtype != MIFFT_F32) {
        why = std::string("the storage type ") + std::to_string(io) + " in the mode word of a " + what +
              " payload: 16-bit rows are widened to float, so the plan must be MIFFT_F32";
        return MIFFT_ERR_BAD_DTYPE;
    }
    p.conv_io = (int)io;
    p.conv_mode = mode & 1u;
    return MIFFT_OK;
}

static int conv_header_check(const Plan& p, const char* tag, std::string& why) {
    const struct {
        uint32_t bits;
        const char* what;
    } other[] = {{MIFFT_FLAG_STFT_POWER, "MIFFT_FLAG_STFT_POWER: a convolution has no magnitude or power store"},
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
    for (const auto& o : other)
        if (p.flags & o.bits) {
            why = std::string("a convolution payload (") + tag + ") with " + o.what;
            return MIFFT_ERR_UNSUPPORTED;
        }
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
    if (!conv_rows_supported(p, n, w)) {
        why = "convolution at an FFT length of " + std::to_string(n) + ": " + w;
        return MIFFT_ERR_UNSUPPORTED;
    }
    return MIFFT_OK;
}

int conv_check(Plan& p, const uint32_t* bases_flat, const int32_t* bases_len, std::vector<uint64_t>& radices,
               std::string& why) {
    if (const int rc = conv_header_check(p, "MIFFT_CONV_TAG", why)) return rc;
    const int64_t L = p.dims[0], n = p.dims[1];
    const bool part = bases_len[0] == 20;  // (partitioned overlap-save: always blocks, F >= 1; word 11 = 0: no gates)
    const bool gated = bases_len[0] == 16 || (part && bases_flat[11] != 0);  // (16 words: word 8 says which form it is, F = 0 the single block)
    const bool ols = bases_len[0] == 12 || part || (gated && bases_flat[8] != 0);  // (overlap-save: rows of T = L samples in blocks of n)
    if (ols && (L < 2 || L > (1ll << 30))) {
        why = "signal rows of T = " + std::to_string(L) + " samples in an overlap-save convolution payload: 2 <= T <= 2^30";
        return L < 2 ? MIFFT_ERR_BAD_DIM : MIFFT_ERR_TOO_LARGE;
    }
    if (!ols && L > n) {
        why = "rows of L = " + std::to_string(L) + " samples are longer than the FFT length n = " + std::to_string(n) +
              " (L > n: rfft(x, n) would crop)";
        return MIFFT_ERR_UNSUPPORTED;
    }
    const int64_t D = bases_flat[2], o = bases_flat[3], Lo = bases_flat[4];
    const uint32_t mode = bases_flat[5];
    const uint64_t addr = (uint64_t)bases_flat[6] | ((uint64_t)bases_flat[7] << 32);
    if (ols) {  // (words 3 and 4 are c and S; Lo is word 10)
        if (Lo < 1 || o + Lo > n) {
            why = "the stored part c = " + std::to_string(o) + ", S = " + std::to_string(Lo) +
                  " of every block of an overlap-save convolution payload: S >= 1 and c + S <= n = " + std::to_string(n);
            return MIFFT_ERR_BAD_BASES;
        }
    } else if (Lo < 1 || o + Lo > n) {
        why = "the output window o = " + std::to_string(o) + ", Lo = " + std::to_string(Lo) +
              " of a convolution payload: Lo >= 1 and o + Lo <= n = " + std::to_string(n);
        return MIFFT_ERR_BAD_BASES;
    }
    if (D < 1) {
        why = "D = 0 filter rows in a convolution payload: D >= 1";
        return MIFFT_ERR_BAD_BASES;
    }
    if (D > (1ll << 30)) {
        why = "D = " + std::to_string(D) + " filter rows: at most 2^30";
        return MIFFT_ERR_TOO_LARGE;
    }
    if (p.batch % D != 0) {
        why = "batch = " + std::to_string(p.batch) + " rows is not a multiple of D = " + std::to_string(D) + " filter rows";
        return MIFFT_ERR_BAD_BATCH;
    }
    if (const int rc = conv_mode_check(p, mode, "convolution", "correlate", why)) return rc;
    if (addr == 0) {
        why = "the filter spectrum address H of a convolution payload is null";
        return MIFFT_ERR_BAD_BASES;
    }
    if (addr % (2 * dtype_size(p.out_dtype)) != 0) {
        why = "the filter spectrum address H of a convolution payload is not aligned to one complex element (" +
              std::to_string(2 * dtype_size(p.out_dtype)) + " bytes)";
        return MIFFT_ERR_BAD_BASES;
    }
    int64_t F = 1, s0 = 0, S = 0, rowLo = Lo;
    if (ols) {
        S = Lo;
        F = bases_flat[8];
        s0 = (int32_t)bases_flat[9];
        rowLo = bases_flat[10];
        if (F < 1 || rowLo < 1) {
            why = "F = " + std::to_string(F) + " blocks and Lo = " + std::to_string(rowLo) +
                  " output samples per row in an overlap-save convolution payload: F >= 1 and Lo >= 1";
            return MIFFT_ERR_BAD_BASES;
        }
        if (rowLo <= (F - 1) * S || rowLo > F * S) {
            why = "Lo = " + std::to_string(rowLo) + " output samples per row against F = " + std::to_string(F) + " blocks of S = " +
                  std::to_string(S) + ": (F - 1) S < Lo <= F S (the last block stores at least one sample)";
            return MIFFT_ERR_BAD_BASES;
        }
        // (partitioned: a block without a live partition stores zeros, so this rule does not apply; Lo is bounded instead)
        if (!part && (s0 <= -n || s0 + (F - 1) * S >= L)) {
            why = "block start s0 = " + std::to_string(s0) + " with F = " + std::to_string(F) + " blocks every S = " +
                  std::to_string(S) + " samples: a block reads no sample of its row (-n < s0 and s0 + (F - 1) S < T = " +
                  std::to_string(L) + ")";
            return MIFFT_ERR_BAD_BASES;
        }
        if (part && rowLo > (1ll << 30)) {
            why = "Lo = " + std::to_string(rowLo) + " output samples per row in a partitioned convolution payload: at most 2^30";
            return MIFFT_ERR_BAD_BASES;
        }
        if (!gated && bases_flat[11] != 0) {
            why = "the reserved word 11 of an overlap-save convolution payload must be 0, not " + std::to_string(bases_flat[11]);
            return MIFFT_ERR_BAD_BASES;
        }
    }
    if (gated) {
        if (!ols && (bases_flat[9] != 0 || bases_flat[10] != 0)) {
            why = "words 9 and 10 (s0 = " + std::to_string(bases_flat[9]) + ", Lo = " + std::to_string(bases_flat[10]) +
                  ") of a gated convolution payload with F = 0 (a single block: o and Lo are words 3 and 4) must be 0";
            return MIFFT_ERR_BAD_BASES;
        }
        if (bases_flat[11] < 1 || bases_flat[11] > 3) {
            why = "the gates word 11 of a gated convolution payload has bit 0 (pregate) and bit 1 (postgate), at least one of them, not " +
                  std::to_string(bases_flat[11]);
            return MIFFT_ERR_BAD_BASES;
        }
        for (int w = 12; w < 16; ++w)
            if (bases_flat[w] != 0) {
                why = "the reserved word " + std::to_string(w) + " of a gated convolution payload must be 0, not " +
                      std::to_string(bases_flat[w]);
                return MIFFT_ERR_BAD_BASES;
            }
    }
    int64_t Q = 0, parts = 0;
    if (part) {
        Q = bases_flat[16];
        parts = bases_flat[17];
        if (Q < 1 || Q > n - 1) {
            why = "Q = " + std::to_string(Q) + " taps per partition in a partitioned convolution payload: 1 <= Q <= n - 1 = " +
                  std::to_string(n - 1);
            return MIFFT_ERR_BAD_BASES;
        }
        if (S > n - Q + 1) {
            why = "S = " + std::to_string(S) + " samples stored per block against Q = " + std::to_string(Q) +
                  " taps per partition: S <= n - Q + 1 = " + std::to_string(n - Q + 1) + " (the rest wraps around)";
            return MIFFT_ERR_BAD_BASES;
        }
        if (parts < 1 || parts * Q > (1ll << 30)) {
            why = "P = " + std::to_string(parts) + " partitions of Q = " + std::to_string(Q) +
                  " taps in a partitioned convolution payload: P >= 1 and P Q <= 2^30";
            return MIFFT_ERR_BAD_BASES;
        }
        for (int w = 12; w < 20; ++w)
            if (w != 16 && w != 17 && bases_flat[w] != 0) {
                why = "the reserved word " + std::to_string(w) + " of a partitioned convolution payload must be 0, not " +
                      std::to_string(bases_flat[w]);
                return MIFFT_ERR_BAD_BASES;
            }
    }
    if (bases_len[1] < 0) {
        why = "negative bases_len";
        return MIFFT_ERR_NO_BASES;
    }
    radices.clear();
    for (int k = 0; k < bases_len[1]; ++k) radices.push_back(bases_flat[bases_len[0] + k]);
    p.conv_D = D;
    p.conv_o = o;
    p.conv_Lo = rowLo;
    p.conv_Q = Q;
    p.conv_parts = parts;
    p.conv_S = S;
    p.conv_F = F;
    p.conv_s0 = s0;
    p.conv_gates = gated ? bases_flat[11] : 0u;
    p.conv_h = (const void*)(uintptr_t)addr;
    return MIFFT_OK;
}

// the one pass: dim 1 (n points) over the rows of the batch; the tables are the half-spectrum row pass's
int build_conv(Plan& p, const std::vector<uint32_t>& ordered, const std::vector<uint32_t>& processed, std::string& why) {
    const int64_t n = p.dims[1];
    DimPass ps;
    ps.dim_index = 1;
    ps.N = n;
    ps.inner = 1;
    ps.outer = p.conv_F;  // (overlap-save: the block rows of one signal row; else 1)
    ps.radices = ordered;
    ps.processed = processed;
    ps.first = true;
    ps.half_pitch = n / 2 + 1;
    if (!select_jit_conv_rows(p, ps, why)) return MIFFT_ERR_UNSUPPORTED;
    hipError_t e = upload_twiddle_table(p.out_dtype, n / 2, false, &ps.d_twiddle);
    if (e == hipSuccess) e = upload_twiddle_table(p.out_dtype, n, false, &ps.d_aux);
    p.passes.push_back(ps);
    if (e != hipSuccess) return hip_error(e, "convolution table upload");
    return MIFFT_OK;
}

// ---- the filter gradient: TAG_LO | TAG_HI | D | c | S | mode | F | s0 | Lo | P | 0 x 6 (MIFFT_CONV_GRAD_TAG, include/mifft.h) ----
bool conv_grad_detect(int ndim, const uint32_t* bases_flat, const int32_t* bases_len) {
    if (ndim != 2 || !bases_flat || !bases_len) return false;
    return bases_len[0] == 16 && bases_flat[0] == MIFFT_CONV_GRAD_TAG_LO && bases_flat[1] == MIFFT_CONV_GRAD_TAG_HI;
}

int conv_grad_check(Plan& p, const uint32_t* bases_flat, const int32_t* bases_len, std::vector<uint64_t>& radices,
                    std::string& why) {
    if (const int rc = conv_header_check(p, "MIFFT_CONV_GRAD_TAG", why)) return rc;
    const int64_t L = p.dims[0], n = p.dims[1];
    const int64_t D = bases_flat[2], c = bases_flat[3], S = bases_flat[4], F = bases_flat[6], s0 = (int32_t)bases_flat[7];
    const int64_t Lo = bases_flat[8], P = bases_flat[9];
    const uint32_t mode = bases_flat[5];
    // (one block that holds the whole row is CONV's geometry; everything else, a single block of a longer row included, OLS's)
    const bool single = F == 1 && s0 == 0 && S == Lo && L <= n;
    if (!single && (L < 2 || L > (1ll << 30))) {
        why = "signal rows of T = " + std::to_string(L) + " samples in an overlap-save filter-gradient payload: 2 <= T <= 2^30";
        return L < 2 ? MIFFT_ERR_BAD_DIM : MIFFT_ERR_TOO_LARGE;
    }
    if (S < 1 || c + S > n) {
        why = "the stored part c = " + std::to_string(c) + ", S = " + std::to_string(S) +
              " of every block of a filter-gradient payload: S >= 1 and c + S <= n = " + std::to_string(n);
        return MIFFT_ERR_BAD_BASES;
    }
    if (D < 1) {
        why = "D = 0 filter rows in a filter-gradient payload: D >= 1";
        return MIFFT_ERR_BAD_BASES;
    }
    if (D > (1ll << 30)) {
        why = "D = " + std::to_string(D) + " filter rows: at most 2^30";
        return MIFFT_ERR_TOO_LARGE;
    }
    if (p.batch % D != 0) {
        why = "batch = " + std::to_string(p.batch) + " rows is not a multiple of D = " + std::to_string(D) + " filter rows";
        return MIFFT_ERR_BAD_BATCH;
    }
    if (const int rc = conv_mode_check(p, mode, "filter-gradient", "the forward correlated", why)) return rc;
    if (F < 1 || Lo < 1 || Lo > (1ll << 30)) {
        why = "F = " + std::to_string(F) + " blocks and Lo = " + std::to_string(Lo) +
              " samples per row of gy in a filter-gradient payload: F >= 1 and 1 <= Lo <= 2^30";
        return MIFFT_ERR_BAD_BASES;
    }
    if (Lo <= (F - 1) * S || Lo > F * S) {
        why = "Lo = " + std::to_string(Lo) + " samples per row of gy against F = " + std::to_string(F) + " blocks of S = " +
              std::to_string(S) + ": (F - 1) S < Lo <= F S (the last block stored at least one sample)";
        return MIFFT_ERR_BAD_BASES;
    }
    if (s0 <= -n || s0 + (F - 1) * S >= L) {
        why = "block start s0 = " + std::to_string(s0) + " with F = " + std::to_string(F) + " blocks every S = " +
              std::to_string(S) + " samples: a block reads no sample of its row (-n < s0 and s0 + (F - 1) S < T = " +
              std::to_string(L) + ")";
        return MIFFT_ERR_BAD_BASES;
    }
    const int64_t pairs = p.batch / D * F;  // (of one channel)
    if (P > 65535 || P > pairs) {
        why = "P = " + std::to_string(P) + " partial sums per channel in a filter-gradient payload: at most 65535 and at most the " +
              std::to_string(pairs) + " (row, block) pairs of a channel (0: the library's choice)";
        return MIFFT_ERR_BAD_BASES;
    }
    for (int w = 10; w < 16; ++w)
        if (bases_flat[w] != 0) {
            why = "the reserved word " + std::to_string(w) + " of a filter-gradient payload must be 0, not " +
                  std::to_string(bases_flat[w]);
            return MIFFT_ERR_BAD_BASES;
        }
    if (bases_len[1] < 0) {
        why = "negative bases_len";
        return MIFFT_ERR_NO_BASES;
    }
    radices.clear();
    for (int k = 0; k < bases_len[1]; ++k) radices.push_back(bases_flat[bases_len[0] + k]);
    p.conv_grad = true;
    p.conv_D = D;
    p.conv_o = c;
    p.conv_Lo = Lo;
    p.conv_S = single ? 0 : S;
    p.conv_F = F;
    p.conv_s0 = s0;
    p.conv_P = P;
    return MIFFT_OK;
}

// P of a built pass when the payload left it to the library: D P workgroups fill the device (as many as the persistent
// grid of a row pass would have), every slice keeps at least one full step of TILE pairs, at most 65535
static int64_t conv_grad_partials(const Plan& p, const DimPass& ps) {
    long long per_cu = (160 * 1024) / (long long)(ps.lds_bytes ? ps.lds_bytes : 1);
    per_cu = std::min<long long>(per_cu, 2048 / ps.threads);
    per_cu = std::max<long long>(1, std::min<long long>(per_cu, 16));
    const int64_t want = (int64_t)p.num_cus * per_cu, pairs = p.batch / p.conv_D * p.conv_F;
    const int64_t P = (want + p.conv_D - 1) / p.conv_D;
    return std::max<int64_t>(1, std::min<int64_t>({P, pairs / ps.tile, (int64_t)65535}));
}

// the one pass, as build_conv's; then P
int build_conv_grad(Plan& p, const std::vector<uint32_t>& ordered, const std::vector<uint32_t>& processed, std::string& why) {
    const int rc = build_conv(p, ordered, processed, why);
    if (rc) return rc;
    if (p.conv_P == 0) p.conv_P = conv_grad_partials(p, p.passes[0]);
    return MIFFT_OK;
}

}  // namespace mifft
