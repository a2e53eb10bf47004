// framed_decode_san.cpp -- the payload decode of the framed plans (MIFFT_FLAG_STFT / MIFFT_FLAG_ISTFT) under the host
// sanitizers, as a program of its own: every payload kind whole, and cut short by one and by two words, through
// mifft_plan_create_slab with device -1.  Each call must come back refused, or with MIFFT_ERR_NO_DEVICE where everything that
// needs no device was accepted, and the sanitizers must stay silent.  Host code only; it never opens a device.
//
//   make -C tools framed_decode_san && tools/hosttests/framed_decode_san
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/mifft.h"

namespace {

void push_f64(std::vector<uint32_t>& w, double v) {
    uint64_t bits;
    memcpy(&bits, &v, sizeof bits);
    w.push_back((uint32_t)bits);
    w.push_back((uint32_t)(bits >> 32));
}

std::vector<uint32_t> window(int n) {
    std::vector<uint32_t> w;
    for (int j = 0; j < n; ++j) push_f64(w, (j + 1) / 16.0);
    return w;
}

struct Case {
    const char* name;
    uint32_t flags;
    int inverse, in_components;
    std::vector<int64_t> dims;
    std::vector<uint32_t> words;
};

int failures = 0;

// the payload in a heap block of exactly its size (a read past its end is the sanitizer's to report), then two radices
void run(const Case& c, int cut) {
    const size_t keep = c.words.size() - (size_t)cut;
    const int ndim = (int)c.dims.size();
    std::unique_ptr<uint32_t[]> flat(new uint32_t[keep + 2]);
    memcpy(flat.get(), c.words.data(), keep * sizeof(uint32_t));
    flat[keep] = 2;
    flat[keep + 1] = 2;
    int32_t lens[3] = {(int32_t)keep, ndim == 3 ? 0 : 2, 2};
    mifft_plan* plan = nullptr;
    const int rc = mifft_plan_create_slab(&plan, /*device=*/-1, MIFFT_F32, MIFFT_F32, ndim, c.dims.data(), /*batch=*/3, c.in_components,
                                          c.inverse, flat.get(), lens, c.flags, 0);
    const bool ok = rc < 0 && plan == nullptr && (cut == 0 || rc != MIFFT_OK);
    printf("%-10s cut %d: status %d (%s)%s\n", c.name, cut, rc, mifft_last_error(), ok ? "" : "   <-- UNEXPECTED");
    if (!ok) ++failures;
    if (cut == 0 && rc != MIFFT_ERR_NO_DEVICE) {
        printf("%-10s whole: expected MIFFT_ERR_NO_DEVICE\n", c.name);
        ++failures;
    }
}

}  // namespace

int main() {
    const int n = 16, hop = 4, T = 100, M = 8, K = n / 2 + 1;
    std::vector<Case> cases;
    const uint32_t H = MIFFT_FLAG_STFT_HOP(hop);
    cases.push_back({"stft", MIFFT_FLAG_STFT | H, 0, 1, {T, n}, window(n)});
    {  // w | power | fb (K, 3)
        std::vector<uint32_t> w = window(n);
        push_f64(w, 2.0);
        for (int i = 0; i < K * 3; ++i) push_f64(w, i / 32.0);
        cases.push_back({"spec", MIFFT_FLAG_STFT | MIFFT_FLAG_STFT_POWER | H, 0, 1, {T, n}, w});
    }
    {  // w | EXT_TAG | power, M, Q, log, add, amin, a, c | fb (K, 3) | post (3, 2)
        std::vector<uint32_t> w = window(n);
        w.push_back(MIFFT_STFT_EXT_TAG_LO);
        w.push_back(MIFFT_STFT_EXT_TAG_HI);
        for (double v : {2.0, 3.0, 2.0, 1.0, 0.0, 1e-10, 0.30102999566398120, 0.0}) push_f64(w, v);
        for (int i = 0; i < K * 3 + 3 * 2; ++i) push_f64(w, (i + 1) / 32.0);
        cases.push_back({"spec-ext", MIFFT_FLAG_STFT | MIFFT_FLAG_STFT_POWER | H, 0, 1, {T, n}, w});
    }
    {  // w | gain
        std::vector<uint32_t> w = window(n);
        push_f64(w, 4.0);
        cases.push_back({"istft", MIFFT_FLAG_ISTFT | H, 1, 2, {T, 22, n}, w});
    }
    {  // w | TAG | gain | mode, 0
        std::vector<uint32_t> w = window(n);
        w.push_back(MIFFT_STFT_ADJ_TAG_LO);
        w.push_back(MIFFT_STFT_ADJ_TAG_HI);
        push_f64(w, 1.0);
        w.push_back(2);
        w.push_back(0);
        cases.push_back({"adjoint", MIFFT_FLAG_ISTFT | H, 1, 2, {T, 22, n}, w});
    }
    for (int inv = 0; inv < 2; ++inv) {  // w | TAG | scale, on either mode bit
        std::vector<uint32_t> w = window(2 * M);
        w.push_back(MIFFT_MDCT_TAG_LO);
        w.push_back(MIFFT_MDCT_TAG_HI);
        push_f64(w, 0.5);
        const uint32_t f = MIFFT_FLAG_STFT_HOP(M) | MIFFT_FLAG_STFT_CENTER_ZEROS;
        if (inv)
            cases.push_back({"imdct", MIFFT_FLAG_ISTFT | f, 1, 1, {T, 14, 2 * M}, w});
        else
            cases.push_back({"mdct", MIFFT_FLAG_STFT | f, 0, 1, {T, 2 * M}, w});
    }
    cases.push_back({"conv", MIFFT_FLAG_STFT, 0, 1, {T, 128}, {MIFFT_CONV_TAG_LO, MIFFT_CONV_TAG_HI, 3, 0, T, 0, 0x1000, 0}});
    cases.push_back({"conv-grad", MIFFT_FLAG_STFT, 0, 1, {T, 128},
                     {MIFFT_CONV_GRAD_TAG_LO, MIFFT_CONV_GRAD_TAG_HI, 3, 0, T, 0, 1, 0, T, 0, 0, 0, 0, 0, 0, 0}});
    for (const Case& c : cases)
        for (int cut = 0; cut <= 2; ++cut) run(c, cut);
    printf(failures ? "%d UNEXPECTED\n" : "all refused or MIFFT_ERR_NO_DEVICE as expected\n", failures);
    return failures ? 1 : 0;
}
