// kernels_dct_rows.hip -- precompiled DCT row kernels of the plans with MIFFT_FLAG_DCT (dct.cpp): TileCfg::DCT = 2 on the
// packed R2C configuration (DCT-II; with and without non-temporal loads of x, the `_ntl` twin of streaming-size tensors) and
// TileCfg::DCT = 3 on the C2R one (its inverse), fp32 and fp64, for rows of 1024 real points.  Each entry is exactly the
// configuration the runtime specialisation would build for that length (kernels_jit.cpp, dct_rows_config), matched by its type
// text as the entries of kernels_half_rows.hip are: 1024-point rows plan without hipRTC (and under MIFFT_JIT=0) with
// bit-identical results.
#include "mifft_internal.h"
#include "tile_kernel.h"

namespace mifft {

#define MIFFT_DCT_ROWS(...) {#__VA_ARGS__, (const void*)&tile_kernel<__VA_ARGS__>, __VA_ARGS__::LDS_BYTES}

static const HalfRowsKernel kDctRows[] = {
    MIFFT_DCT_ROWS(mifft::TileCfg<float, 512, 3, 8, 8, 8, 1, 8, 256, false, false, false, 2, 1, false, 0, false, false, 0, false, float, false, false, 0, false, false, true, false, 0, 2>),  // rows1024_dct2_8x8x8
    MIFFT_DCT_ROWS(mifft::TileCfg<float, 512, 3, 8, 8, 8, 1, 8, 256, false, false, false, 2, 1, false, 0, false, false, 1, false, float, false, false, 0, false, false, true, false, 0, 2>),  // rows1024_dct2_8x8x8_ntl
    MIFFT_DCT_ROWS(mifft::TileCfg<float, 512, 3, 8, 8, 8, 1, 8, 256, false, false, false, 2, 1, false, 0, false, false, 0, false, float, false, false, 0, false, false, false, true, 0, 3>),  // rows1024_dct3_8x8x8
    MIFFT_DCT_ROWS(mifft::TileCfg<double, 512, 3, 8, 8, 8, 1, 4, 256, false, false, false, 2, 1, false, 0, false, false, 0, false, double, false, false, 0, false, false, true, false, 0, 2>),  // rows1024_f64_dct2_8x8x8
    MIFFT_DCT_ROWS(mifft::TileCfg<double, 512, 3, 8, 8, 8, 1, 4, 256, false, false, false, 2, 1, false, 0, false, false, 1, false, double, false, false, 0, false, false, true, false, 0, 2>),  // rows1024_f64_dct2_8x8x8_ntl
    MIFFT_DCT_ROWS(mifft::TileCfg<double, 512, 3, 8, 8, 8, 1, 4, 256, false, false, false, 2, 1, false, 0, false, false, 0, false, double, false, false, 0, false, false, false, true, 0, 3>),  // rows1024_f64_dct3_8x8x8
};

const HalfRowsKernel* dct_rows_kernels(int* count) {
    *count = (int)(sizeof kDctRows / sizeof kDctRows[0]);
    return kDctRows;
}

}  // namespace mifft
