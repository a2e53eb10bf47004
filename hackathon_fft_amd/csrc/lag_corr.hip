// lag_corr.hip -- stage 2 of the fused partitioned filter gradient (conv.cpp, ConvRequest::stage = 3): the lag-group
// correlation over the half spectra that stage 1 (TileCfg::WSPEC, tile_kernel.h) left in memory.
//
// U is (rows, Fu, bins) and G (rows, F, bins), complex values of the plan's float type, rows = B D, bins = n / 2 + 1; stored
// frame j of U is u-frame m0 + j, every other frame counts as zeros and is never read.  For every channel d, lag group
// p < Pg and bin k,
//     A[d][p][k] = sum over b, ascending, and over f < F, ascending, of conj(U[b, d, f - p][k]) G[b, d, f][k]
// (the forward correlated: U[b, d, f + p], and the conjugate of the sum is stored).  Work items run along k, so consecutive
// items load consecutive bins with one 8-byte (double: 16-byte) load each; a workgroup owns a channel, kLagCorrThreads bins
// and a contiguous slice of the batch, and stores row (slice, d, p) of `out` once, unscaled.  Every item keeps Pg complex
// accumulators and a sliding window of the last Pg frames of U in registers -- slot s holds U[f + lead - s], lead = 0
// (correlation: Pg - 1), so that a step of f shifts the window by one slot and loads ONE new frame: every value of U and of
// G is loaded once per workgroup.  The register arrays have a compile-time bound PB in {2, 4, 8, 16, 32} >= Pg and are
// indexed by unrolled constants only.  No LDS, no atomics; the order of every sum is fixed by (B, P), so two runs give the
// same bits.
#include <algorithm>

#include "mifft_internal.h"

namespace mifft {

namespace {

template <typename T> struct C2;
template <> struct C2<float> { using type = float2; };
template <> struct C2<double> { using type = double2; };

struct LagCorrParams {
    const void* U;
    const void* G;
    void* out;
    int bins, xblocks;  // n / 2 + 1; ceil(bins / kLagCorrThreads)
    int D, B, P;        // channels, batch entries per channel, slices of them
    int Pg, F, Fu, m0;  // lag groups, g-blocks per row, stored u-frames per row, the frame index of the first
    int corr;
};

template <typename T, int PB>
__global__ __launch_bounds__(kLagCorrThreads) void lag_corr_kernel(const LagCorrParams p) {
    using V = typename C2<T>::type;
    // workgroup -> (slice, channel, bin group), the bin group fastest
    const int xb = (int)(blockIdx.x % (unsigned)p.xblocks);
    const long long rest = (long long)(blockIdx.x / (unsigned)p.xblocks);
    const int d = (int)(rest % p.D), sl = (int)(rest / p.D);
    const int k = xb * kLagCorrThreads + (int)threadIdx.x;
    if (k >= p.bins) return;
    const int len = p.B / p.P, rem = p.B - len * p.P;
    int b = sl * len + (sl < rem ? sl : rem);
    const int b_end = b + len + (sl < rem ? 1 : 0);
    const int Pg = p.Pg, F = p.F, Fu = p.Fu, m0 = p.m0, bins = p.bins;
    const int lead = p.corr ? Pg - 1 : 0;
    V acc[PB], win[PB];
#pragma unroll
    for (int s = 0; s < PB; ++s) acc[s] = V{(T)0, (T)0};
    for (; b < b_end; ++b) {
        const long long row = (long long)b * p.D + d;
        const V* const u = (const V*)p.U + row * Fu * bins + k;
        const V* const g = (const V*)p.G + row * F * bins + k;
        // u-frame m of the row: stored frame m - m0, or zeros (never read)
        auto frame = [&](int m) -> V {
            const int j = m - m0;
            return j >= 0 && j < Fu ? u[(long long)j * bins] : V{(T)0, (T)0};
        };
        // the window of f = 0, but for its newest frame: slot s holds U[lead - s]
#pragma unroll
        for (int s = 1; s < PB; ++s) win[s] = s < Pg ? frame(lead - s) : V{(T)0, (T)0};
        for (int f = 0; f < F; ++f) {
            win[0] = frame(f + lead);
            const V gv = g[(long long)f * bins];
#pragma unroll
            for (int s = 0; s < PB; ++s) {  // conj(U) G
                acc[s].x += win[s].x * gv.x + win[s].y * gv.y;
                acc[s].y += win[s].x * gv.y - win[s].y * gv.x;
            }
#pragma unroll
            for (int s = PB - 1; s >= 1; --s) win[s] = win[s - 1];
        }
    }
    // slot s is lag group s (correlation: Pg - 1 - s); row (slice, d, p) of bins values
    const T cj = p.corr ? (T)-1 : (T)1;
    V* const out = (V*)p.out + ((long long)sl * p.D + d) * Pg * bins + k;
#pragma unroll
    for (int s = 0; s < PB; ++s)
        if (s < Pg) {
            const int pg = p.corr ? Pg - 1 - s : s;
            out[(long long)pg * bins] = V{acc[s].x, acc[s].y * cj};
        }
}

int lag_corr_bound(int lag_groups) {
    for (int pb = 2; pb < 32; pb *= 2)
        if (lag_groups <= pb) return pb;
    return 32;
}

template <typename T>
hipError_t launch_bound(int pb, unsigned grid, hipStream_t stream, const LagCorrParams& p) {
    switch (pb) {
        case 2: hipLaunchKernelGGL((lag_corr_kernel<T, 2>), dim3(grid), dim3(kLagCorrThreads), 0, stream, p); break;
        case 4: hipLaunchKernelGGL((lag_corr_kernel<T, 4>), dim3(grid), dim3(kLagCorrThreads), 0, stream, p); break;
        case 8: hipLaunchKernelGGL((lag_corr_kernel<T, 8>), dim3(grid), dim3(kLagCorrThreads), 0, stream, p); break;
        case 16: hipLaunchKernelGGL((lag_corr_kernel<T, 16>), dim3(grid), dim3(kLagCorrThreads), 0, stream, p); break;
        default: hipLaunchKernelGGL((lag_corr_kernel<T, 32>), dim3(grid), dim3(kLagCorrThreads), 0, stream, p); break;
    }
    return hipGetLastError();
}

int64_t lag_corr_xblocks(const Plan& plan) { return (plan.dims[1] / 2 + 1 + kLagCorrThreads - 1) / kLagCorrThreads; }

}  // namespace

const char* lag_corr_kernel_name(int dtype, int lag_groups) {
    static const char* const names[2][5] = {
        {"lag_corr_f32_p2", "lag_corr_f32_p4", "lag_corr_f32_p8", "lag_corr_f32_p16", "lag_corr_f32_p32"},
        {"lag_corr_f64_p2", "lag_corr_f64_p4", "lag_corr_f64_p8", "lag_corr_f64_p16", "lag_corr_f64_p32"}};
    int i = 0;
    for (int pb = 2; pb < lag_corr_bound(lag_groups); pb *= 2) ++i;
    return names[dtype == MIFFT_F64 ? 1 : 0][i];
}

int64_t lag_corr_partials(const Plan& plan) {
    const int64_t D = plan.conv.D, B = plan.batch / D, wgs = D * lag_corr_xblocks(plan);
    const int64_t want = (int64_t)plan.num_cus * 4;  // (256 work items each: a wave per SIMD from every one of four workgroups)
    if (wgs >= want) return 1;
    return std::max<int64_t>(1, std::min<int64_t>({(want + wgs - 1) / wgs, B, (int64_t)65535}));
}

int launch_lag_corr(const Plan& plan, const void* U, const void* G, void* out, hipStream_t stream) {
    const ConvRequest& cv = plan.conv;
    LagCorrParams p;
    p.U = U;
    p.G = G;
    p.out = out;
    p.bins = (int)(plan.dims[1] / 2 + 1);
    p.xblocks = (int)lag_corr_xblocks(plan);
    p.D = (int)cv.D;
    p.B = (int)(plan.batch / cv.D);
    p.P = (int)cv.P;
    p.Pg = (int)cv.lag_groups;
    p.F = (int)cv.F;
    p.Fu = (int)cv.u_frames;
    p.m0 = (int)cv.u_first;
    p.corr = (int)(cv.mode & 1u);
    const long long grid = (long long)p.xblocks * p.D * p.P;
    if (grid > 0x7fffffffll) return set_error(MIFFT_ERR_TOO_LARGE, "lag-group correlation: more than 2^31 - 1 workgroups");
    const int pb = lag_corr_bound(p.Pg);
    const hipError_t e = plan.out_dtype == MIFFT_F64 ? launch_bound<double>(pb, (unsigned)grid, stream, p)
                                                     : launch_bound<float>(pb, (unsigned)grid, stream, p);
    if (e != hipSuccess) return hip_error(e, "lag_corr_kernel launch");
    return MIFFT_OK;
}

}  // namespace mifft
