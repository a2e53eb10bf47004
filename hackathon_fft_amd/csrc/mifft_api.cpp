// mifft_api.cpp -- the C ABI of libmifft (see include/mifft.h): plan creation as a dispatcher over the routes (the general
// one: schedule.cpp), execution, introspection.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <optional>

#include "mifft_config.h"
#include "mifft_internal.h"

namespace mifft {

static thread_local std::string g_last_error;

int set_error(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

int hip_error(hipError_t e, const char* what) {
    g_last_error = std::string("HIP error: ") + hipGetErrorString(e) + " in " + what;
    return MIFFT_ERR_HIP;
}

size_t Plan::in_elem_bytes() const { return dtype_size(in_dtype) * (size_t)in_components; }
size_t Plan::out_elem_bytes() const { return dtype_size(out_dtype) * 2; }
size_t Plan::in_row_bytes() const {
    if (stft() && conv.is_conv()) return (size_t)dims[0] * conv.elem_bytes(out_dtype);  // (rows of the storage type)
    if (stft()) return (size_t)dims[0] * dtype_size(in_dtype);
    if (istft()) return (size_t)prod_half * in_elem_bytes();
    if (dct_any()) return (size_t)prod * dtype_size(in_dtype);
    return (size_t)(half_spectrum() && inverse ? prod_half : prod) * in_elem_bytes();
}
size_t Plan::out_row_bytes() const {
    if (stft() && conv.gradient()) return 0;  // (the result is no row per batch entry: mifft_plan_out_bytes)
    if (stft() && conv.is_conv()) return (size_t)conv.Lo * conv.elem_bytes(out_dtype);
    if (stft() && mdct) return (size_t)(stft_frames() * mdct) * dtype_size(out_dtype);
    if (stft() && spec_power) return (size_t)(stft_frames() * stft_out_width()) * dtype_size(out_dtype);
    if (stft()) return (size_t)prod_half * out_elem_bytes();
    if (istft()) return (size_t)dims[0] * dtype_size(out_dtype);
    if (dct_any()) return (size_t)prod * dtype_size(out_dtype);
    if (!half_spectrum()) return (size_t)prod * out_elem_bytes();
    return inverse ? (size_t)prod * dtype_size(out_dtype) : (size_t)prod_half * out_elem_bytes();
}
size_t Plan::scratch_row_bytes() const { return (size_t)(half_spectrum() ? prod_half : prod) * out_elem_bytes(); }

// W_N^n = exp(-+ 2*pi*i*n/N), evaluated in long double and rounded once to the
// output dtype (reference formula: fft/fft/_utils.mojo:63-104, which rounds theta
// to the working dtype first; see DESIGN.md "numerics").
template <typename T>
static void fill_twiddles(std::vector<T>& tab, int64_t N, bool inverse) {
    tab.resize((size_t)2 * N);
    const long double two_pi = 6.283185307179586476925286766559005768L;
    for (int64_t n = 0; n < N; ++n) {
        // exact octant values where they exist
        long double re, im;
        const int64_t n8 = 8 * n;
        if (n8 % N == 0 && ((n8 / N) % 2) == 0) {
            switch ((n8 / N) / 2) {
                case 0: re = 1, im = 0; break;
                case 1: re = 0, im = -1; break;
                case 2: re = -1, im = 0; break;
                default: re = 0, im = 1; break;
            }
        } else {
            long double th = -two_pi * (long double)n / (long double)N;
            re = cosl(th);
            im = sinl(th);
        }
        if (inverse) im = -im;
        tab[2 * n] = (T)re;
        tab[2 * n + 1] = (T)im;
    }
}

hipError_t upload_twiddle_table(int out_dtype, int64_t N, bool inverse, void** d_table) {
    hipError_t err;
    if (out_dtype == MIFFT_F32) {
        std::vector<float> tab;
        fill_twiddles(tab, N, inverse);
        err = hipMalloc(d_table, tab.size() * sizeof(float));
        if (err == hipSuccess) err = hipMemcpy(*d_table, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice);
    } else {
        std::vector<double> tab;
        fill_twiddles(tab, N, inverse);
        err = hipMalloc(d_table, tab.size() * sizeof(double));
        if (err == hipSuccess) err = hipMemcpy(*d_table, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice);
    }
    return err;
}

// Switches to the plan's device for the duration of a call and restores the caller's current device
// afterwards (the library must not leave a side effect on the host framework's device state).
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int device) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != device) {
            err = hipSetDevice(device);
            switched = err == hipSuccess;
        }
    }
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
};

// The exec of a gated convolution plan (conv.cpp; ConvRequest::gates): the `x` of mifft_exec / mifft_exec_batch is the HOST
// address of a mifft_gated_args, which names x and the gates of this exec.  Refused without a launch: a device address (the
// signal itself, as an ungated plan takes it) or a block without the magic word, MIFFT_ERR_UNSUPPORTED; a gate the plan has
// and the block lacks, MIFFT_ERR_NULL; a gate the plan did not ask for, MIFFT_ERR_UNSUPPORTED.  On success `x` is the signal.
static int unpack_gated_args(const Plan& p, const void*& x, const void*& pregate, const void*& postgate) {
    static const char* kHow =
        "the exec of a gated convolution plan takes the host address of a mifft_gated_args (magic, x, pregate, postgate) in "
        "the place of x: include/mifft.h";
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, x) != hipSuccess)
        (void)hipGetLastError();  // (memory the runtime has never seen: host memory)
    else if (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeArray)
        return set_error(MIFFT_ERR_UNSUPPORTED, std::string("x is a device address: ") + kHow);
    const mifft_gated_args* g = (const mifft_gated_args*)x;
    if (g->magic != MIFFT_GATED_ARGS_MAGIC) return set_error(MIFFT_ERR_UNSUPPORTED, std::string("no magic word: ") + kHow);
    if (!g->x) return set_error(MIFFT_ERR_NULL, "mifft_gated_args.x is NULL");
    const bool want_a = p.conv.gates & 1u, want_b = p.conv.gates & 2u;
    if (want_a && !g->pregate) return set_error(MIFFT_ERR_NULL, "the plan has a pregate (gates bit 0): mifft_gated_args.pregate is NULL");
    if (want_b && !g->postgate) return set_error(MIFFT_ERR_NULL, "the plan has a postgate (gates bit 1): mifft_gated_args.postgate is NULL");
    if (!want_a && g->pregate) return set_error(MIFFT_ERR_UNSUPPORTED, "mifft_gated_args.pregate is set, but the plan has no pregate (gates bit 0)");
    if (!want_b && g->postgate) return set_error(MIFFT_ERR_UNSUPPORTED, "mifft_gated_args.postgate is set, but the plan has no postgate (gates bit 1)");
    x = g->x;
    pregate = g->pregate;
    postgate = g->postgate;
    return MIFFT_OK;
}

// The exec of a filter-gradient plan (conv.cpp; ConvRequest::grad): `x` is the HOST address of a mifft_conv_grad_args, refused
// without a launch as above.  On success `x` and `gy` are the two inputs.  A plan with gates (word 11 of its payload) takes a
// mifft_conv_grad_gated_args, a block with a magic word of its own, instead -- the old block, which has no room for a gate, is
// refused as a block without the magic word is -- and the gate rules are unpack_gated_args's.
static int unpack_conv_grad_args(const Plan& p, const void*& x, const void*& gy, const void*& pregate, const void*& postgate) {
    static const char* kHow =
        "the exec of a filter-gradient plan takes the host address of a mifft_conv_grad_args (magic, x, gy) in the place of "
        "x: include/mifft.h";
    static const char* kHowGated =
        "the exec of a gated filter-gradient plan takes the host address of a mifft_conv_grad_gated_args (magic, x, gy, pregate, "
        "postgate) in the place of x: include/mifft.h";
    const bool gated = p.conv.gated();
    const char* how = gated ? kHowGated : kHow;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, x) != hipSuccess)
        (void)hipGetLastError();  // (memory the runtime has never seen: host memory)
    else if (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeArray)
        return set_error(MIFFT_ERR_UNSUPPORTED, std::string("x is a device address: ") + how);
    pregate = postgate = nullptr;
    if (!gated) {
        const mifft_conv_grad_args* g = (const mifft_conv_grad_args*)x;
        if (g->magic != MIFFT_CONV_GRAD_ARGS_MAGIC) return set_error(MIFFT_ERR_UNSUPPORTED, std::string("no magic word: ") + how);
        if (!g->x && p.conv.stage != 2) return set_error(MIFFT_ERR_NULL, "mifft_conv_grad_args.x is NULL");
        if (!g->gy && p.conv.stage != 1) return set_error(MIFFT_ERR_NULL, "mifft_conv_grad_args.gy is NULL");
        gy = g->gy;
        x = g->x;
        return MIFFT_OK;
    }
    const mifft_conv_grad_gated_args* g = (const mifft_conv_grad_gated_args*)x;  // (the magic word is the first member of both)
    if (g->magic == MIFFT_CONV_GRAD_ARGS_MAGIC)
        return set_error(MIFFT_ERR_UNSUPPORTED, std::string("a mifft_conv_grad_args names no gates: ") + how);
    if (g->magic != MIFFT_CONV_GRAD_GATED_ARGS_MAGIC) return set_error(MIFFT_ERR_UNSUPPORTED, std::string("no magic word: ") + how);
    if (!g->x && p.conv.stage != 2) return set_error(MIFFT_ERR_NULL, "mifft_conv_grad_gated_args.x is NULL");
    if (!g->gy && p.conv.stage != 1) return set_error(MIFFT_ERR_NULL, "mifft_conv_grad_gated_args.gy is NULL");
    const bool want_a = p.conv.gates & 1u, want_b = p.conv.gates & 2u;
    if (want_a && !g->pregate)
        return set_error(MIFFT_ERR_NULL, "the plan has a pregate (gates bit 0): mifft_conv_grad_gated_args.pregate is NULL");
    if (want_b && !g->postgate)
        return set_error(MIFFT_ERR_NULL, "the plan has a postgate (gates bit 1): mifft_conv_grad_gated_args.postgate is NULL");
    if (!want_a && g->pregate)
        return set_error(MIFFT_ERR_UNSUPPORTED, "mifft_conv_grad_gated_args.pregate is set, but the plan has no pregate (gates bit 0)");
    if (!want_b && g->postgate)
        return set_error(MIFFT_ERR_UNSUPPORTED, "mifft_conv_grad_gated_args.postgate is set, but the plan has no postgate (gates bit 1)");
    gy = g->gy;
    pregate = g->pregate;
    postgate = g->postgate;
    x = g->x;
    return MIFFT_OK;
}

// the bytes of a filter-gradient plan's result: (P D, n / 2 + 1) complex values; the spectra of stage 1 or 2: (batch, F, n / 2 + 1);
// the lag-group sums of stage 3: (P D Pg, n / 2 + 1)
static size_t conv_grad_out_bytes(const Plan& p) {
    const size_t line = (size_t)(p.dims[1] / 2 + 1) * 2 * dtype_size(p.out_dtype);
    if (p.conv.stage == 1 || p.conv.stage == 2) return (size_t)p.batch * (size_t)p.conv.F * line;
    if (p.conv.stage == 3) return (size_t)(p.conv.P * p.conv.D * p.conv.lag_groups) * line;
    return (size_t)(p.conv.P * p.conv.D) * line;
}

// the bytes of the two inputs of such an exec (0: the stage does not read that one)
static size_t conv_grad_x_bytes(const Plan& p) {
    if (p.conv.stage == 2) return 0;
    if (p.conv.stage == 3) return (size_t)p.batch * (size_t)p.conv.u_frames * (size_t)(p.dims[1] / 2 + 1) * 2 * dtype_size(p.out_dtype);
    return (size_t)p.batch * p.in_row_bytes();
}
static size_t conv_grad_gy_bytes(const Plan& p) {
    if (p.conv.stage == 1) return 0;
    if (p.conv.stage == 3) return (size_t)p.batch * (size_t)p.conv.F * (size_t)(p.dims[1] / 2 + 1) * 2 * dtype_size(p.out_dtype);
    return (size_t)p.batch * (size_t)p.conv.Lo * p.conv.elem_bytes(p.out_dtype);
}

static int exec_conv_grad(const Plan& p, const void* x, void* out, int64_t first, int64_t count, void* stream) {
    if (first != 0 || count != p.batch)
        return set_error(MIFFT_ERR_BAD_BATCH, "the exec of a filter-gradient plan covers the whole batch (first = 0, count = batch): "
                                              "a slab would be a partial sum");
    const void *gy = nullptr, *pregate = nullptr, *postgate = nullptr;
    if (const int rc = unpack_conv_grad_args(p, x, gy, pregate, postgate)) return rc;
    const char *xb = (const char*)x, *gb = (const char*)gy, *ob = (const char*)out;
    const size_t xn = conv_grad_x_bytes(p), gn = conv_grad_gy_bytes(p), on = conv_grad_out_bytes(p);
    if (xn && xb < ob + on && ob < xb + xn) return set_error(MIFFT_ERR_ALIAS, "x and out must not overlap");
    if (gn && gb < ob + on && ob < gb + gn) return set_error(MIFFT_ERR_ALIAS, "gy and out must not overlap");
    // (the pregate has x's size, the postgate gy's; either may alias x, gy or the other: none is written)
    const char *ab = (const char*)pregate, *bb = (const char*)postgate;
    if (ab && ab < ob + on && ob < ab + xn) return set_error(MIFFT_ERR_ALIAS, "the pregate and out must not overlap");
    if (bb && bb < ob + on && ob < bb + gn) return set_error(MIFFT_ERR_ALIAS, "the postgate and out must not overlap");
    DeviceGuard guard(p.device);
    MIFFT_HIP_TRY(guard.err);
    if (p.conv.stage == 3) return launch_lag_corr(p, x, gy, out, (hipStream_t)stream);  // (x: the spectra U, gy: the spectra G)
    return launch_jit_conv_grad(p, p.passes[0], x, gy, pregate, postgate, out, (hipStream_t)stream);
}

// The exec of a two-signal convolution plan (conv.cpp; ConvRequest::pair): `args` is the HOST address of a mifft_conv_pair_args,
// refused without a launch as above.  first / count offset x, v and out by whole rows of L, K and Lo samples.  x and v may be
// the same buffer; neither may overlap the exec's part of out.
static int exec_conv_pair(const Plan& p, const void* args, void* out, int64_t first, int64_t count, void* stream) {
    static const char* kHow =
        "the exec of a two-signal convolution plan takes the host address of a mifft_conv_pair_args (magic, x, v) in the place "
        "of x: include/mifft.h";
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, args) != hipSuccess)
        (void)hipGetLastError();  // (memory the runtime has never seen: host memory)
    else if (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeArray)
        return set_error(MIFFT_ERR_UNSUPPORTED, std::string("x is a device address: ") + kHow);
    const mifft_conv_pair_args* a = (const mifft_conv_pair_args*)args;
    if (a->magic != MIFFT_CONV_PAIR_ARGS_MAGIC) return set_error(MIFFT_ERR_UNSUPPORTED, std::string("no magic word: ") + kHow);
    if (!a->x) return set_error(MIFFT_ERR_NULL, "mifft_conv_pair_args.x is NULL");
    if (!a->v) return set_error(MIFFT_ERR_NULL, "mifft_conv_pair_args.v is NULL");
    const size_t x_row = p.in_row_bytes(), v_row = (size_t)p.conv.K * p.conv.elem_bytes(p.out_dtype), o_row = p.out_row_bytes();
    const char* xb = (const char*)a->x + (size_t)first * x_row;
    const char* vb = (const char*)a->v + (size_t)first * v_row;
    char* ob = (char*)out + (size_t)first * o_row;
    const size_t xn = (size_t)count * x_row, vn = (size_t)count * v_row, on = (size_t)count * o_row;
    if (xb < ob + on && ob < xb + xn) return set_error(MIFFT_ERR_ALIAS, "x and out must not overlap");
    if (vb < ob + on && ob < vb + vn) return set_error(MIFFT_ERR_ALIAS, "v and out must not overlap");
    DeviceGuard guard(p.device);
    MIFFT_HIP_TRY(guard.err);
    return launch_jit_conv_pair(p, p.passes[0], xb, vb, ob, count, (hipStream_t)stream);
}

// The exec of an STFT adjoint plan (istft.cpp; Plan::stft_adj): `x` is the HOST address of a mifft_stft_adj_args, refused
// without a launch as above.  x is the gradient (mode 1) or X (modes 2, 3); mult is present exactly for modes 2 and 3, edge
// exactly with the reflect bit.  first / count offset all four tensors by whole entries.
static int exec_stft_adj(const Plan& p, const void* args, void* out, int64_t first, int64_t count, void* stream) {
    static const char* kHow =
        "the exec of an STFT adjoint plan takes the host address of a mifft_stft_adj_args (magic, x, mult, edge) in the place "
        "of x: include/mifft.h";
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, args) != hipSuccess)
        (void)hipGetLastError();  // (memory the runtime has never seen: host memory)
    else if (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeArray)
        return set_error(MIFFT_ERR_UNSUPPORTED, std::string("x is a device address: ") + kHow);
    const mifft_stft_adj_args* a = (const mifft_stft_adj_args*)args;
    if (a->magic != MIFFT_STFT_ADJ_ARGS_MAGIC) return set_error(MIFFT_ERR_UNSUPPORTED, std::string("no magic word: ") + kHow);
    if (!a->x) return set_error(MIFFT_ERR_NULL, "mifft_stft_adj_args.x is NULL");
    const bool want_m = p.stft_adj >= 2, want_e = p.stft_adj_edges();
    if (want_m && !a->mult)
        return set_error(MIFFT_ERR_NULL, "the STFT adjoint plan has a factor (mode 2 or 3): mifft_stft_adj_args.mult is NULL");
    if (want_e && !a->edge)
        return set_error(MIFFT_ERR_NULL, "the STFT adjoint plan stores the reflected edges (MIFFT_FLAG_STFT_CENTER_REFLECT): "
                                         "mifft_stft_adj_args.edge is NULL");
    if (!want_m && a->mult)
        return set_error(MIFFT_ERR_UNSUPPORTED, "mifft_stft_adj_args.mult is set, but the STFT adjoint plan has no factor (mode 1)");
    if (!want_e && a->edge)
        return set_error(MIFFT_ERR_UNSUPPORTED, "mifft_stft_adj_args.edge is set, but the STFT adjoint plan stores no edges (no "
                                                "MIFFT_FLAG_STFT_CENTER_REFLECT)");
    const size_t esz = dtype_size(p.out_dtype);
    const size_t x_row = p.in_row_bytes(), m_row = (size_t)p.prod_half * esz, o_row = p.out_row_bytes(), e_row = (size_t)p.dims[2] * esz;
    const char* xb = (const char*)a->x + (size_t)first * x_row;
    const char* mb = a->mult ? (const char*)a->mult + (size_t)first * m_row : nullptr;
    char* ob = (char*)out + (size_t)first * o_row;
    char* eb = a->edge ? (char*)a->edge + (size_t)first * e_row : nullptr;
    const size_t xn = (size_t)count * x_row, mn = (size_t)count * m_row, on = (size_t)count * o_row, en = (size_t)count * e_row;
    auto overlap = [](const char* r, size_t rn, const char* w, size_t wn) { return r && w && r < w + wn && w < r + rn; };
    if (overlap(xb, xn, ob, on)) return set_error(MIFFT_ERR_ALIAS, "x and out must not overlap");
    if (overlap(mb, mn, ob, on)) return set_error(MIFFT_ERR_ALIAS, "mult and out must not overlap");
    if (overlap(xb, xn, eb, en)) return set_error(MIFFT_ERR_ALIAS, "x and edge must not overlap");
    if (overlap(mb, mn, eb, en)) return set_error(MIFFT_ERR_ALIAS, "mult and edge must not overlap");
    if (overlap(eb, en, ob, on)) return set_error(MIFFT_ERR_ALIAS, "edge and out must not overlap");
    DeviceGuard guard(p.device);
    MIFFT_HIP_TRY(guard.err);
    return launch_stft_adj(p, p.passes[0], xb, mb, ob, eb, count, (hipStream_t)stream);
}

static int device_count_quiet() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

}  // namespace mifft

using namespace mifft;

// ---- plan creation: one owner for the handle, one place each for the header and the device ----
namespace {

// Owns the handle until plan creation hands it out (release()): every error return frees whatever the plan has uploaded so
// far.  free_plan_device makes no HIP call for a plan that owns nothing, so the early, device-less refusals cost none.
struct PlanDeleter {
    void operator()(mifft_plan* h) const { free_plan_device(h->p); delete h; }
};
using PlanOwner = std::unique_ptr<mifft_plan, PlanDeleter>;

// a route builder's status: MIFFT_ERR_HIP has been recorded (with the HIP message) where it arose
int fail(int rc, const std::string& why) { return rc == MIFFT_ERR_HIP ? rc : set_error(rc, why); }

// The plan header from the arguments of plan creation; what follows reads them from the plan.  prod / prod_half are those of
// a full transform of dims; the framed route replaces them with its own.
void fill_header(Plan& p, int device, int in_dtype, int out_dtype, int ndim, const int64_t* dims, int64_t batch,
                 int64_t whole_batch, int in_components, int inverse, uint32_t flags) {
    p.device = device;
    p.in_dtype = in_dtype;
    p.out_dtype = out_dtype;
    p.ndim = ndim;
    p.batch = batch;
    p.sel_batch = whole_batch;
    p.in_components = in_components;
    p.inverse = inverse ? 1 : 0;
    p.flags = flags;
    p.prod = 1;
    for (int i = 0; i < ndim; ++i) {
        p.dims[i] = dims[i];
        p.prod *= dims[i];
    }
    p.prod_half = p.prod / dims[ndim - 1] * (dims[ndim - 1] / 2 + 1);
}

// The plan's device: refused when it is not a usable one, else made current through `guard`, which the caller holds until plan
// creation returns (it must outlive the PlanOwner, whose deleter frees device memory).
int open_device(Plan& p, std::optional<DeviceGuard>& guard) {
    const int ndev = device_count_quiet();
    if (p.device < 0 || p.device >= ndev)
        return set_error(MIFFT_ERR_NO_DEVICE, "libmifft has no CPU path: device " + std::to_string(p.device) +
                                                  " is not a usable HIP device (" + std::to_string(ndev) + " visible)");
    guard.emplace(p.device);
    if (guard->err != hipSuccess) return hip_error(guard->err, "hipSetDevice");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, p.device) == hipSuccess) p.num_cus = prop.multiProcessorCount;
    config_refresh();  // (lab builds re-read their MIFFT_* switches per plan; a no-op in the product library)
    return MIFFT_OK;
}

// STFT and inverse STFT plans (MIFFT_FLAG_STFT, stft.cpp; MIFFT_FLAG_ISTFT, istft.cpp) and the MDCT / IMDCT / fused
// convolution plans (conv.cpp) their tagged payloads select: their own route to the end.  Everything that can be refused
// without a device first; `bases` carries the window and the radices of the one transformed dim, the last.
FramedKind framed_kind(const Plan& p, const uint32_t* bases_flat, const int32_t* bases_len) {
    if (p.stft()) {  // (both mode bits as well: stft_check refuses the pair)
        // a payload that STARTS with MIFFT_CONV_GRAD_TAG: the filter gradient of a fused FFT convolution; with MIFFT_CONV_TAG:
        // that convolution, of rows of dims[0] samples at length dims[1]
        if (conv_grad_detect(p.ndim, bases_flat, bases_len)) return FramedKind::ConvGrad;
        // ... with MIFFT_CONV_PAIR_TAG: the convolution of two signal batches, row by row
        if (conv_pair_detect(p.ndim, bases_flat, bases_len)) return FramedKind::ConvPair;
        if (conv_detect(p.ndim, bases_flat, bases_len)) return FramedKind::Conv;
        // a window payload tagged with MIFFT_MDCT_TAG: the MDCT, M = n / 2 coefficients per frame from a DCT-IV of M points
        if (mdct_detect(p.ndim, p.dims, bases_flat, bases_len)) return FramedKind::Mdct;
        // ... or with MIFFT_ISTFT_ADJ_TAG (no power bit: there that slot is the power's): the adjoint of the inverse STFT
        if (!(p.flags & MIFFT_FLAG_STFT_POWER) && istft_adj_detect(p.ndim, p.dims, bases_flat, bases_len)) return FramedKind::IstftAdjoint;
        return FramedKind::Stft;
    }
    // the window of a MIFFT_FLAG_ISTFT plan tagged with MIFFT_STFT_ADJ_TAG: the adjoint of the STFT, the ISTFT pass without
    // envelope; with MIFFT_MDCT_TAG: the inverse MDCT, frames of M = n / 2 coefficients overlap-added every M samples
    if (stft_adj_detect(p.ndim, p.dims, bases_flat, bases_len)) return FramedKind::Adjoint;
    if (imdct_detect(p.ndim, bases_flat, bases_len)) return FramedKind::Imdct;
    return FramedKind::Istft;
}

int create_framed(Plan& p, const uint32_t* bases_flat, const int32_t* bases_len, std::optional<DeviceGuard>& guard) {
    const int ndim = p.ndim;
    const int64_t* dims = p.dims;
    const FramedKind kind = framed_kind(p, bases_flat, bases_len);
    std::string why;
    FramedPayload pl;
    int rc = MIFFT_OK;
    switch (kind) {
        case FramedKind::ConvGrad: rc = conv_grad_check(p, bases_flat, bases_len, pl, why); break;
        case FramedKind::Conv: rc = conv_check(p, bases_flat, bases_len, pl, why); break;
        case FramedKind::ConvPair: rc = conv_pair_check(p, bases_flat, bases_len, pl, why); break;
        case FramedKind::Mdct: rc = mdct_check(p, bases_flat, bases_len, pl, why); break;
        case FramedKind::Imdct: rc = imdct_check(p, bases_flat, bases_len, pl, why); break;
        case FramedKind::Adjoint: rc = stft_adj_check(p, bases_flat, bases_len, pl, why); break;
        case FramedKind::IstftAdjoint: rc = istft_adj_check(p, bases_flat, bases_len, pl, why); break;
        case FramedKind::Stft: rc = stft_check(p, why); break;
        case FramedKind::Istft: rc = istft_check(p, bases_flat, bases_len, pl, why); break;
    }
    if (rc) return fail(rc, why);
    const int td = ndim - 1;  // the transformed dim
    const bool lapped = kind == FramedKind::Mdct || kind == FramedKind::Imdct;
    const int64_t n = lapped ? dims[td] / 4 : dims[td], frames = p.stft() ? p.stft_frames() : dims[1];  // (MDCT: M / 2 complex points)
    p.prod = frames * (kind == FramedKind::Mdct ? p.mdct : kind == FramedKind::Imdct ? p.imdct : n);  // (the rows the one pass transforms)
    p.prod_half = lapped ? p.prod : frames * (n / 2 + 1);
    if (kind == FramedKind::Stft) {
        rc = stft_unpack_bases(p, bases_flat, bases_len, pl, why);
        if (rc) return fail(rc, why);
    }
    if (pl.radices.empty()) pl.radices = plan_estimate_bases((uint64_t)n, /*gpu_target=*/true);
    std::vector<std::vector<uint32_t>> ordered((size_t)ndim), processed((size_t)ndim);
    rc = plan_ordered_bases((uint64_t)n, pl.radices, ordered[td], processed[td], why);
    if (rc) return fail(rc, why);
    p.stage_radices = ordered;  // (the other dims are framed / overlap-added, not transformed: no stages)
    rc = open_device(p, guard);
    if (rc) return rc;
    switch (kind) {
        case FramedKind::ConvGrad: rc = build_conv_grad(p, ordered[td], processed[td], why); break;
        case FramedKind::ConvPair:  // (the convolution's pass, with TileCfg::PAIR)
        case FramedKind::Conv: rc = build_conv(p, ordered[td], processed[td], why); break;
        case FramedKind::Mdct: rc = build_mdct(p, ordered[td], processed[td], pl, why); break;
        case FramedKind::Imdct: rc = build_imdct(p, ordered[td], processed[td], pl, why); break;
        case FramedKind::Stft: rc = build_stft(p, ordered[td], processed[td], pl, why); break;
        case FramedKind::IstftAdjoint: rc = build_istft_adj(p, ordered[td], processed[td], pl, why); break;
        case FramedKind::Adjoint:  // (the inverse STFT's pass, without the envelope)
        case FramedKind::Istft: rc = build_istft(p, ordered[td], processed[td], pl, why); break;
    }
    return rc ? fail(rc, why) : MIFFT_OK;
}

// DCT plans (MIFFT_FLAG_DCT, dct.cpp; MIFFT_FLAG_DCT_ND, dctn.cpp) and kept dimensions (MIFFT_FLAG_KEEP_DIM; axes.cpp):
// everything that can be refused without a device, the DCT checks before the keep bits are looked at.  Sets p.dct4 and p.dst.
int dct_and_keep_check(Plan& p, const uint32_t* bases_flat, const int32_t* bases_len) {
    const uint32_t flags = p.flags;
    if ((flags & MIFFT_FLAG_DCT_ORTHO) && !(flags & (MIFFT_FLAG_DCT | MIFFT_FLAG_DCT_ND)))
        return set_error(MIFFT_ERR_UNSUPPORTED, "MIFFT_FLAG_DCT_ORTHO without MIFFT_FLAG_DCT or MIFFT_FLAG_DCT_ND");
    // (a MIFFT_FLAG_DCT plan whose first `bases` word is MIFFT_DCT_TYPE4_TAG is a DCT-IV; the radices of n / 2 follow the tag)
    const bool tagged = bases_flat && bases_len && bases_len[0] >= 1 && bases_flat[0] == MIFFT_DCT_TYPE4_TAG;
    if ((flags & MIFFT_FLAG_DCT_ND) && tagged)
        return set_error(MIFFT_ERR_UNSUPPORTED, "MIFFT_DCT_TYPE4_TAG with MIFFT_FLAG_DCT_ND: the N-D DCT has no type 4");
    // (MIFFT_DST_TAG / MIFFT_DST_TYPE4_TAG in the same place: the sine transform of that type on the DCT plan's passes)
    const uint32_t word0 = bases_flat && bases_len && bases_len[0] >= 1 ? bases_flat[0] : 0u;
    const bool dst2 = word0 == MIFFT_DST_TAG, dst4 = word0 == MIFFT_DST_TYPE4_TAG;
    if ((flags & MIFFT_FLAG_DCT_ND) && dst4)
        return set_error(MIFFT_ERR_UNSUPPORTED, "MIFFT_DST_TYPE4_TAG with MIFFT_FLAG_DCT_ND: the N-D DST has no type 4");
    p.dct4 = (flags & MIFFT_FLAG_DCT) && (tagged || dst4);
    p.dst = ((flags & MIFFT_FLAG_DCT) && (dst2 || dst4)) || ((flags & MIFFT_FLAG_DCT_ND) && dst2);
    if (p.dct_any()) {
        std::string why;
        const int rc = p.dct_nd() ? dctn_check(p, why) : dct_check(p, why);
        if (rc) return set_error(rc, why);
    }
    const uint32_t keep = p.keep_mask();
    if (!keep) return MIFFT_OK;
    if (keep >> p.ndim)
        return set_error(MIFFT_ERR_BAD_DIM, "MIFFT_FLAG_KEEP_DIM names a dimension at or beyond ndim (" + std::to_string(p.ndim) + ")");
    if (keep == (1u << p.ndim) - 1u) return set_error(MIFFT_ERR_BAD_DIM, "every dimension is kept: no dimension to transform");
    if (flags & MIFFT_FLAG_FAITHFUL_STAGES)
        return set_error(MIFFT_ERR_UNSUPPORTED,
                         "MIFFT_FLAG_KEEP_DIM with MIFFT_FLAG_FAITHFUL_STAGES: the reference has no axes to be faithful to");
    if (bases_len)
        for (int i = 0; i < p.ndim; ++i)
            if (p.kept(i) && bases_len[i] != (p.dst && i == 0 ? 1 : 0))  // (a kept dimension 0 still carries MIFFT_DST_TAG, alone)
                return set_error(MIFFT_ERR_BAD_BASES, "dimension " + std::to_string(i) + " is kept: its bases_len must be 0");
    return MIFFT_OK;
}

// radix planning per dimension (host only; errors before any device use)
int plan_radices(const Plan& p, const uint32_t* bases_flat, const int32_t* bases_len,
                 std::vector<std::vector<uint32_t>>& ordered, std::vector<std::vector<uint32_t>>& processed) {
    const uint32_t* bp = bases_flat;
    for (int i = 0; i < p.ndim; ++i) {
        if (p.kept(i)) {  // (no stages: mifft_plan_stages() reports 0)
            if (bases_flat && p.dst && i == 0) ++bp;  // (the tag)
            continue;
        }
        std::vector<uint64_t> user;
        if (bases_flat) {
            if (bases_len[i] < 0) return set_error(MIFFT_ERR_NO_BASES, "negative bases_len");
            for (int k = 0; k < bases_len[i]; ++k) user.push_back(*bp++);
            if ((p.dct4 || p.dst) && i == 0) user.erase(user.begin());  // (the tag; alone it selects the default estimate, below)
        } else {
            user = plan_estimate_bases((uint64_t)p.dims[i], /*gpu_target=*/true);
        }
        std::string err;
        // (a DCT plan runs, and reports, the stages of its packed n / 2-point transform: for its rows, the last dimension)
        const bool packed = p.dct() || (p.dct_nd() && i == p.ndim - 1);
        if (packed && (!bases_flat || (p.dct4 && user.empty()))) user = plan_estimate_bases((uint64_t)p.dims[i] / 2, /*gpu_target=*/true);
        // (a DST plan always has a `bases` argument, for its tag: an empty list there is the default of that dimension)
        if (bases_flat && p.dst && user.empty()) user = plan_estimate_bases((uint64_t)p.dims[i] / (packed ? 2 : 1), /*gpu_target=*/true);
        const int rc = plan_ordered_bases((uint64_t)p.dims[i] / (packed ? 2 : 1), user, ordered[i], processed[i], err);
        if (rc) return set_error(rc, err);
    }
    return MIFFT_OK;
}

// 32-bit lane offsets of the column tiles (tile_kernel.h, lane_off): a strided dimension must span fewer than 2^32 elements,
// N * stride < 2^32 (a single transform of more than 32 GB; checked before any device work)
int lane_offset_check(const Plan& p) {
    double inner = 1.0;
    for (int i = p.ndim - 1; i >= 0; --i) {
        if (i < p.ndim - 1 && !p.kept(i) && (double)p.dims[i] * inner + 64.0 >= 4294967296.0)
            return set_error(MIFFT_ERR_TOO_LARGE,
                             "dimension " + std::to_string(i) + " (" + std::to_string(p.dims[i]) + " points at stride " +
                                 std::to_string((long long)inner) + ") spans 2^32 elements or more: strided tiles "
                                 "address their elements with 32-bit lane offsets");
        inner *= (double)p.dims[i];
    }
    return MIFFT_OK;
}

// Infinity-Cache policy for N-D transforms (thresholds: mifft_config.h).  Bit 0 of nd_mode = the first pass reads x with
// non-temporal loads when `out` fits the 256-MiB cache, so that x does not displace the row results the next pass reads
// (100 x 640 x 480: rows 96.2 -> 92.6 us, columns 102.9 -> 88.1 us); bit 1 = in-place passes walk their tiles in alternating
// directions, starting with the lines written last (build_general; 10 x 128^3: 0.131 -> 0.128 ms, 100 x 64^3 with both:
// 0.151 -> 0.139 ms).  Results are bit-identical in every mode.
void set_cache_policy(Plan& p) {
    const Config& cfg = config();
    const double out_bytes = p.size_batch() * (double)p.prod * (double)p.out_elem_bytes();
    // ... and only when x and out together do NOT fit: below ~160 MB per tensor everything stays cache-resident
    // between the passes (and between execs), and non-temporal loads of x cost 6-9 % (100-image batches of
    // 640 x 480 at 59 / 118 MB: 0.0510 -> 0.0551 / 0.0834 -> 0.0905 ms, 64^3 the same; tools/nd_size_probe.py)
    p.cache_resident_nd = p.ndim >= 2 && (cfg.nd_mode & 1) && out_bytes <= cfg.nd_out_max_bytes && out_bytes >= cfg.nd_out_min_bytes;
}

}  // namespace

// The library is built with -fvisibility=hidden: ONLY the C ABI below is exported.  (Its internal C++ names live in namespace
// mifft; exported, they would interpose with equally named symbols of the program that loads the library.)
#pragma GCC visibility push(default)
extern "C" {

const char* mifft_last_error(void) { return g_last_error.c_str(); }

const char* mifft_status_string(int s) {
    switch (s) {
        case MIFFT_OK: return "ok";
        case MIFFT_ERR_BAD_RANK: return "bad rank";
        case MIFFT_ERR_BAD_DIM: return "bad dimension";
        case MIFFT_ERR_BAD_COMPONENTS: return "bad component count";
        case MIFFT_ERR_BAD_DTYPE: return "bad dtype";
        case MIFFT_ERR_BAD_BASES: return "bases do not factor the length";
        case MIFFT_ERR_BASE_ONE: return "base 1";
        case MIFFT_ERR_NO_BASES: return "no bases";
        case MIFFT_ERR_BAD_BATCH: return "bad batch";
        case MIFFT_ERR_TOO_LARGE: return "dimension too large";
        case MIFFT_ERR_NO_DEVICE: return "no device";
        case MIFFT_ERR_HIP: return "hip error";
        case MIFFT_ERR_NULL: return "null argument";
        case MIFFT_ERR_ALIAS: return "x and out overlap";
        case MIFFT_ERR_BUFFER_TOO_SMALL: return "buffer too small";
        case MIFFT_ERR_UNSUPPORTED: return "unsupported request";
    }
    return "unknown";
}

int mifft_version(void) { return MIFFT_VERSION_MAJOR * 100 + MIFFT_VERSION_MINOR; }

int mifft_device_count(void) { return device_count_quiet(); }

int mifft_ordered_bases(uint32_t length, const uint32_t* bases, int nbases, uint32_t* ordered_out, int capacity) {
    std::vector<uint64_t> user;
    for (int i = 0; i < nbases; ++i) user.push_back(bases[i]);
    std::vector<uint32_t> ord, proc;
    std::string err;
    int rc = plan_ordered_bases(length, user, ord, proc, err);
    if (rc) return set_error(rc, err);
    for (size_t i = 0; i < ord.size() && (int)i < capacity; ++i) ordered_out[i] = ord[i];
    return (int)ord.size();
}

int mifft_estimate_bases(uint32_t length, int target_gpu, uint32_t* bases_out, int capacity) {
    if (length < 2) return set_error(MIFFT_ERR_BAD_DIM, "length must be >= 2");
    auto b = plan_estimate_bases(length, target_gpu != 0);
    for (size_t i = 0; i < b.size() && (int)i < capacity; ++i) bases_out[i] = (uint32_t)b[i];
    return (int)b.size();
}

int mifft_plan_create(mifft_plan** out_plan, int device, int in_dtype, int out_dtype, int ndim,
                      const int64_t* dims, int64_t batch, int in_components, int inverse,
                      const uint32_t* bases_flat, const int32_t* bases_len, uint32_t flags) {
    return mifft_plan_create_slab(out_plan, device, in_dtype, out_dtype, ndim, dims, batch, in_components, inverse,
                                  bases_flat, bases_len, flags, 0);
}

int mifft_plan_create_slab(mifft_plan** out_plan, int device, int in_dtype, int out_dtype, int ndim,
                           const int64_t* dims, int64_t batch, int in_components, int inverse,
                           const uint32_t* bases_flat, const int32_t* bases_len, uint32_t flags,
                           int64_t whole_batch) {
    if (!out_plan) return set_error(MIFFT_ERR_NULL, "out_plan is NULL");
    *out_plan = nullptr;
    if (whole_batch != 0 && whole_batch < batch) return set_error(MIFFT_ERR_BAD_BATCH, "whole_batch must be 0 or >= batch");
    // ---- validation = _check_layout_conditions_nd (fft/fft/fft.mojo:20-46) ----
    if (ndim < 1 || ndim > MIFFT_MAX_DIMS)
        return set_error(MIFFT_ERR_BAD_RANK, "The rank should be bigger than 2 (1..6 transformed dims supported)");
    if (!dims) return set_error(MIFFT_ERR_NULL, "dims is NULL");
    if (in_components < 1 || in_components > 2)
        return set_error(MIFFT_ERR_BAD_COMPONENTS, "The last dimension of in_layout should be 1 or 2");
    if (out_dtype != MIFFT_F32 && out_dtype != MIFFT_F64)
        return set_error(MIFFT_ERR_BAD_DTYPE, "out_dtype must be floating point");
    if (dtype_size(in_dtype) == 0) return set_error(MIFFT_ERR_BAD_DTYPE, "unsupported in_dtype");
    if (batch < 0) return set_error(MIFFT_ERR_BAD_BATCH, "batch must be >= 0");
    for (int i = 0; i < ndim; ++i) {
        if (i == 1 && ndim == 3 && (flags & MIFFT_FLAG_ISTFT) && dims[i] == 1) continue;  // (one frame: istft.cpp)
        if (dims[i] < 2) return set_error(MIFFT_ERR_BAD_DIM, "no inner dimension should be of size 1");
    }
    if ((bases_flat == nullptr) != (bases_len == nullptr))
        return set_error(MIFFT_ERR_NULL, "bases_flat and bases_len must both be given or both be NULL");
    std::string why;
    int rc = stft_flag_check(flags, why);
    if (rc) return set_error(rc, why);

    std::optional<DeviceGuard> guard;  // (before the owner: the owner's deleter frees device memory under it)
    PlanOwner h(new mifft_plan());
    Plan& p = h->p;
    fill_header(p, device, in_dtype, out_dtype, ndim, dims, batch, whole_batch, in_components, inverse, flags);
    if (flags & (MIFFT_FLAG_STFT | MIFFT_FLAG_ISTFT)) {
        rc = create_framed(p, bases_flat, bases_len, guard);
        if (rc) return rc;
        *out_plan = h.release();
        return MIFFT_OK;
    }
    // ---- what can be refused without a device is refused here: DCT and keep bits, radices, lane offsets, masked and
    //      half-spectrum plans (an N-D DCT plan's own check has covered its lengths) ----
    std::vector<std::vector<uint32_t>> ordered(ndim), processed(ndim);
    if ((rc = dct_and_keep_check(p, bases_flat, bases_len)) || (rc = plan_radices(p, bases_flat, bases_len, ordered, processed)) ||
        (rc = lane_offset_check(p)))
        return rc;
    if (p.keep_mask() && !p.dct_nd() && (rc = axes_check(p, why))) return set_error(rc, why);
    if (p.half_spectrum() && (rc = half_spectrum_check(p, why))) return set_error(rc, why);
    // ---- device, cache policy, then the passes in execution order (last dimension first) by the plan's route: the masked,
    //      half-spectrum and DCT plans have their own (axes.cpp, half_spectrum.cpp, dct.cpp, dctn.cpp), every other plan the
    //      general one (schedule.cpp) ----
    if ((rc = open_device(p, guard))) return rc;
    set_cache_policy(p);
    p.stage_radices = ordered;
    rc = p.dct()              ? build_dct(p, ordered[0], processed[0], why)
         : p.dct_nd()         ? build_dctn(p, ordered, processed, why)
         : p.keep_mask()      ? build_axes(p, ordered, processed, why)
         : p.half_spectrum()  ? build_half_spectrum(p, ordered, processed, why)
                              : build_general(p, ordered, processed, why);
    if (rc) return fail(rc, why);
    *out_plan = h.release();
    return MIFFT_OK;
}

int mifft_exec_batch(const mifft_plan* plan, const void* x, void* out, int64_t first, int64_t count,
                     void* stream) {
    if (!plan) return set_error(MIFFT_ERR_NULL, "plan is NULL");
    const Plan& p = plan->p;
    if (first < 0 || count < 0 || first + count > p.batch)
        return set_error(MIFFT_ERR_BAD_BATCH, "batch range out of bounds");
    if (p.conv.gradient()) {  // (`x`: the HOST address of the exec's mifft_conv_grad_args; the whole batch or nothing)
        if (!x || !out) return set_error(MIFFT_ERR_NULL, "x or out is NULL");
        return exec_conv_grad(p, x, out, first, count, stream);
    }
    if (count == 0) return MIFFT_OK;
    if (!x || !out) return set_error(MIFFT_ERR_NULL, "x or out is NULL");
    if (p.stft_adj) return exec_stft_adj(p, x, out, first, count, stream);  // (`x`: the HOST address of the exec's mifft_stft_adj_args)
    if (p.conv.pair) return exec_conv_pair(p, x, out, first, count, stream);  // (`x`: the HOST address of the exec's mifft_conv_pair_args)
    const void *pregate = nullptr, *postgate = nullptr;
    if (p.conv.gated()) {  // (a gated convolution: `x` is the HOST address of the exec's mifft_gated_args)
        const int rc = unpack_gated_args(p, x, pregate, postgate);  // (x: now the signal itself)
        if (rc) return rc;
    }
    const size_t in_row = p.in_row_bytes(), out_row = p.out_row_bytes();
    const char* xb = (const char*)x + (size_t)first * in_row;
    char* ob = (char*)out + (size_t)first * out_row;
    // out-of-place contract (reference: first stage reads x, all writes go elsewhere)
    if (xb < ob + (size_t)count * out_row && ob < xb + (size_t)count * in_row)
        return set_error(MIFFT_ERR_ALIAS, "x and out must not overlap");
    // (the gates of the exec's rows: the pregate is offset like x, the postgate like out; either may alias x, neither out)
    const char* ab = pregate ? (const char*)pregate + (size_t)first * in_row : nullptr;
    const char* bb = postgate ? (const char*)postgate + (size_t)first * out_row : nullptr;
    if (ab && ab < ob + (size_t)count * out_row && ob < ab + (size_t)count * in_row)
        return set_error(MIFFT_ERR_ALIAS, "the pregate and out must not overlap");
    if (bb && bb < ob + (size_t)count * out_row && ob < bb + (size_t)count * out_row)
        return set_error(MIFFT_ERR_ALIAS, "the postgate and out must not overlap");
    DeviceGuard guard(p.device);
    MIFFT_HIP_TRY(guard.err);
    hipStream_t s = (hipStream_t)stream;
    char* sb = p.d_scratch ? (char*)p.d_scratch + (size_t)first * p.scratch_row_bytes() : nullptr;
    auto buf = [&](int which) -> char* { return which == 0 ? (char*)xb : which == 2 ? sb : ob; };
    if (p.conv.is_conv()) return launch_jit_conv(p, p.passes[0], xb, ob, ab, bb, first, count, s);  // (the filter row of row i: (first + i) % D)
    for (const DimPass& ps : p.passes) {
        const void* src = ps.src_buf >= 0 ? buf(ps.src_buf) : (ps.first ? (const char*)xb : ob);
        void* dst = ps.dst_buf >= 0 ? buf(ps.dst_buf) : ob;
        int rc = ps.launch(p, ps, src, dst, count, s);
        if (rc) return rc;
    }
    return MIFFT_OK;
}

int mifft_exec(const mifft_plan* plan, const void* x, void* out, void* stream) {
    if (!plan) return set_error(MIFFT_ERR_NULL, "plan is NULL");
    return mifft_exec_batch(plan, x, out, 0, plan->p.batch, stream);
}

void mifft_plan_destroy(mifft_plan* plan) {
    if (!plan) return;
    {
        DeviceGuard guard(plan->p.device);
        free_plan_device(plan->p);
    }
    delete plan;
}

int mifft_plan_stages(const mifft_plan* plan, int dim, uint32_t* radices_out, int capacity) {
    if (!plan) return set_error(MIFFT_ERR_NULL, "plan is NULL");
    if (dim < 0 || dim >= plan->p.ndim) return set_error(MIFFT_ERR_BAD_RANK, "dim out of range");
    const std::vector<uint32_t>& r = plan->p.stage_radices[dim];
    for (size_t i = 0; i < r.size() && (int)i < capacity; ++i) radices_out[i] = r[i];
    return (int)r.size();
}

const char* mifft_plan_kernel_name(const mifft_plan* plan, int dim) {
    if (!plan) return "";
    if (dim >= 0 && dim < plan->p.ndim && plan->p.kept(dim)) return "none";
    if (dim == 0 && plan->p.stft()) return "none";  // (framed, not transformed)
    if (dim >= 0 && dim < 2 && plan->p.istft()) return "none";  // (samples and frames: overlap-added, not transformed)
    for (const DimPass& ps : plan->p.passes)
        if (ps.dim_index == dim || ps.dim_index2 == dim) return ps.kernel_name;
    return "";
}

int mifft_plan_pass_geometry(const mifft_plan* plan, int dim, int64_t count, int64_t geometry_out[4]) {
    if (!plan || !geometry_out) return set_error(MIFFT_ERR_NULL, "plan or geometry_out is NULL");
    if (dim < 0 || dim >= plan->p.ndim) return set_error(MIFFT_ERR_BAD_RANK, "dim out of range");
    if (count < 1) return set_error(MIFFT_ERR_BAD_BATCH, "count must be positive");
    if (plan->p.kept(dim)) return set_error(MIFFT_ERR_UNSUPPORTED, "a kept dim has no pass");
    if (dim == 0 && plan->p.stft()) return set_error(MIFFT_ERR_UNSUPPORTED, "dim 0 of an STFT plan is framed: it has no pass");
    if (dim < 2 && plan->p.istft())
        return set_error(MIFFT_ERR_UNSUPPORTED, "dims 0 and 1 of an inverse STFT plan are overlap-added: they have no pass");
    const DimPass* found = nullptr;
    for (const DimPass& ps : plan->p.passes)
        if (ps.dim_index == dim || ps.dim_index2 == dim) {
            if (found) return set_error(MIFFT_ERR_UNSUPPORTED, "the dimension takes more than one launch");
            found = &ps;
        }
    if (!found || found->dim_index2 >= 0 || !tile_pass_geometry(plan->p, *found, count, geometry_out))
        return set_error(MIFFT_ERR_UNSUPPORTED, std::string("pass \"") + (found ? found->kernel_name : "none") +
                                                    "\" is not one persistent tile_kernel launch");
    return MIFFT_OK;
}

int mifft_plan_num_launches(const mifft_plan* plan) {
    if (!plan) return set_error(MIFFT_ERR_NULL, "plan is NULL");
    return (int)plan->p.passes.size();
}

size_t mifft_plan_in_bytes(const mifft_plan* plan) {
    if (plan && plan->p.stft_adj >= 2)  // (X and the real factor beside it)
        return (size_t)plan->p.batch * (plan->p.in_row_bytes() + (size_t)plan->p.prod_half * dtype_size(plan->p.out_dtype));
    return plan ? (size_t)plan->p.batch * plan->p.in_row_bytes() : 0;
}

size_t mifft_plan_out_bytes(const mifft_plan* plan) {
    if (plan && plan->p.conv.gradient()) return conv_grad_out_bytes(plan->p);
    if (plan && plan->p.stft_adj_edges())  // (the signal's gradient and the two edge strips of n / 2 samples)
        return (size_t)plan->p.batch * (plan->p.out_row_bytes() + (size_t)plan->p.dims[2] * dtype_size(plan->p.out_dtype));
    return plan ? (size_t)plan->p.batch * plan->p.out_row_bytes() : 0;
}

size_t mifft_plan_scratch_bytes(const mifft_plan* plan) { return plan && plan->p.d_scratch ? plan->p.scratch_bytes : 0; }

int mifft_plan_device_status(const mifft_plan* plan, void* stream, uint32_t* flags_out) {
    if (!plan || !flags_out) return set_error(MIFFT_ERR_NULL, "plan or flags_out is NULL");
    *flags_out = 0;
    DeviceGuard guard(plan->p.device);
    MIFFT_HIP_TRY(guard.err);
    for (const DimPass& ps : plan->p.passes) {
        if (!ps.needs_counters || !ps.d_aux2) continue;
        hipStream_t s = (hipStream_t)stream;
        unsigned v = 0;
        MIFFT_HIP_TRY(hipMemcpyAsync(&v, (const unsigned*)ps.d_aux2 + 16, sizeof v, hipMemcpyDeviceToHost, s));
        MIFFT_HIP_TRY(hipMemsetAsync((unsigned*)ps.d_aux2 + 16, 0, sizeof v, s));
        MIFFT_HIP_TRY(hipStreamSynchronize(s));
        *flags_out |= v;
    }
    return MIFFT_OK;
}

int mifft_time_exec(const mifft_plan* plan, const void* x, void* out, void* stream, int iters, float* ms_out) {
    if (!plan || !ms_out) return set_error(MIFFT_ERR_NULL, "plan or ms_out is NULL");
    if (iters < 1) iters = 1;
    DeviceGuard guard(plan->p.device);
    MIFFT_HIP_TRY(guard.err);
    hipStream_t s = (hipStream_t)stream;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t he = hipEventCreate(&e0);
    if (he == hipSuccess) he = hipEventCreate(&e1);
    int rc = MIFFT_OK;
    if (he == hipSuccess) he = hipEventRecord(e0, s);
    for (int i = 0; i < iters && rc == MIFFT_OK && he == hipSuccess; ++i) rc = mifft_exec(plan, x, out, stream);
    if (he == hipSuccess) he = hipEventRecord(e1, s);
    if (he == hipSuccess) he = hipEventSynchronize(e1);
    float ms = 0.f;
    if (he == hipSuccess) he = hipEventElapsedTime(&ms, e0, e1);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (rc) return rc;
    if (he != hipSuccess) return hip_error(he, "mifft_time_exec events");
    *ms_out = ms / (float)iters;
    return MIFFT_OK;
}

int mifft_jit_precompile(int in_dtype, int out_dtype, int64_t length, int strided, int real_input,
                         size_t* code_bytes_out) {
    if (dtype_size(in_dtype) == 0) return set_error(MIFFT_ERR_BAD_DTYPE, "unknown in dtype");
    if (out_dtype != MIFFT_F32 && out_dtype != MIFFT_F64) return set_error(MIFFT_ERR_BAD_DTYPE, "out dtype must be f32 or f64");
    if (length < 2) return set_error(MIFFT_ERR_BAD_DIM, "length must be >= 2");
    std::string why;
    const int rc = jit_precompile(in_dtype, out_dtype, length, strided, real_input, code_bytes_out, why);
    if (rc != MIFFT_OK) return set_error(rc, why);
    return MIFFT_OK;
}

}  // extern "C"
#pragma GCC visibility pop
