// kernels_half_rows.hip -- precompiled packed real-row kernels of the half-spectrum plans (MIFFT_FLAG_HALF_SPECTRUM,
// half_spectrum.cpp): TileCfg::R2C (forward; with and without non-temporal loads of x, the `_ntl` twin of cache-resident N-D
// plans) and TileCfg::C2R (inverse), fp32 and fp64, for the last dimensions of the BASELINE / reference-bench shapes
// (128, 480, 1024, 1080, 1920 real points).  Each entry is exactly the configuration the runtime specialisation would build
// for that length (kernels_jit.cpp, packed_rows_config): select_jit_half_rows matches the configuration's type text against
// this table first, so these lengths plan without hipRTC (and under MIFFT_JIT=0) with bit-identical results.  The type text
// of an entry is its own instantiation (stringified), so the two cannot drift apart.
#include "mifft_internal.h"
#include "tile_kernel.h"

namespace mifft {

#define MIFFT_HALF_ROWS(...) {#__VA_ARGS__, (const void*)&tile_kernel<__VA_ARGS__>, __VA_ARGS__::LDS_BYTES}

static const HalfRowsKernel kHalfRows[] = {
    MIFFT_HALF_ROWS(mifft::TileCfg<float, 64, 2, 8, 8, 1, 1, 64, 256, false, true, false, 2, 1, false, 0, false, false, 0, false, float, false, false, 0, false, false, true>),  // rows128_r2c_8x8
    MIFFT_HALF_ROWS(mifft::TileCfg<float, 64, 2, 8, 8, 1, 1, 64, 256, false, true, false, 2, 1, false, 0, false, false, 1, false, float, false, false, 0, false, false, true>),  // rows128_r2c_8x8_ntl
    MIFFT_HALF_ROWS(mifft::TileCfg<float, 64, 2, 8, 8, 1, 1, 64, 256, false, false, false, 2, 1, false, 0, false, false, 0, false, float, false, false, 0, false, false, false, true>),  // rows128_c2r_8x8
    MIFFT_HALF_ROWS(mifft::TileCfg<float, 240, 2, 16, 15, 1, 1, 17, 256, false, true, false, 2, 1, false, 0, false, false, 0, false, float, false, false, 0, false, false, true>),  // rows480_r2c_16x15
    MIFFT_HALF_ROWS(mifft::TileCfg<float, 240, 2, 16, 15, 1, 1, 17, 256, false, true, false, 2, 1, false, 0, false, false, 1, false, float, false, false, 0, false, false, true>),  // rows480_r2c_16x15_ntl
    MIFFT_HALF_ROWS(mifft::TileCfg<float, 240, 2, 16, 15, 1, 1, 17, 256, false, false, true, 2, 1, false, 0, false, false, 0, false, float, false, false, 0, false, false, false, true>),  // rows480_c2r_16x15
    MIFFT_HALF_ROWS(mifft::TileCfg<float, 512, 3, 8, 8, 8, 1, 8, 256, false, true, false, 2, 1, false, 0, false, false, 0, false, float, false, false, 0, false, false, true>),  // rows1024_r2c_8x8x8
    MIFFT_HALF_ROWS(mifft::TileCfg<float, 512, 3, 8, 8, 8, 1, 8, 256, false, true, false, 2, 1, false, 0, false, false, 1, false, float, false, false, 0, false, false, true>),  // rows1024_r2c_8x8x8_ntl
    MIFFT_HALF_ROWS(mifft::TileCfg<float, 512, 3, 8, 8, 8, 1, 8, 256, false, false, true, 2, 1, false, 0, false, false, 0, false, float, false, false, 0, false, false, false, true>),  // rows1024_c2r_8x8x8
    MIFFT_HALF_ROWS(mifft::TileCfg<float, 540, 3, 10, 9, 6, 1, 7, 256, false, true, false, 2, 1, false, 0, false, false, 0, false, float, false, false, 0, false, false, true>),  // rows1080_r2c_10x9x6
    MIFFT_HALF_ROWS(mifft::TileCfg<float, 540, 3, 10, 9, 6, 1, 7, 256, false, true, false, 2, 1, false, 0, false, false, 1, false, float, false, false, 0, false, false, true>),  // rows1080_r2c_10x9x6_ntl
    MIFFT_HALF_ROWS(mifft::TileCfg<float, 540, 3, 10, 9, 6, 1, 7, 256, false, false, true, 2, 1, false, 0, false, false, 0, false, float, false, false, 0, false, false, false, true>),  // rows1080_c2r_10x9x6
    MIFFT_HALF_ROWS(mifft::TileCfg<float, 960, 3, 12, 10, 8, 1, 4, 256, false, true, false, 2, 1, false, 0, false, false, 0, false, float, false, false, 0, false, false, true>),  // rows1920_r2c_12x10x8
    MIFFT_HALF_ROWS(mifft::TileCfg<float, 960, 3, 12, 10, 8, 1, 4, 256, false, true, false, 2, 1, false, 0, false, false, 1, false, float, false, false, 0, false, false, true>),  // rows1920_r2c_12x10x8_ntl
    MIFFT_HALF_ROWS(mifft::TileCfg<float, 960, 3, 12, 10, 8, 1, 4, 256, false, false, true, 2, 1, false, 0, false, false, 0, false, float, false, false, 0, false, false, false, true>),  // rows1920_c2r_12x10x8
    MIFFT_HALF_ROWS(mifft::TileCfg<double, 64, 2, 8, 8, 1, 1, 32, 256, false, true, false, 2, 1, false, 0, false, false, 0, false, double, false, false, 0, false, false, true>),  // rows128_f64_r2c_8x8
    MIFFT_HALF_ROWS(mifft::TileCfg<double, 64, 2, 8, 8, 1, 1, 32, 256, false, true, false, 2, 1, false, 0, false, false, 1, false, double, false, false, 0, false, false, true>),  // rows128_f64_r2c_8x8_ntl
    MIFFT_HALF_ROWS(mifft::TileCfg<double, 64, 2, 8, 8, 1, 1, 32, 256, false, false, false, 2, 1, false, 0, false, false, 0, false, double, false, false, 0, false, false, false, true>),  // rows128_f64_c2r_8x8
    MIFFT_HALF_ROWS(mifft::TileCfg<double, 240, 3, 8, 6, 5, 1, 8, 256, false, true, false, 2, 1, false, 0, false, false, 0, false, double, false, false, 0, false, false, true>),  // rows480_f64_r2c_8x6x5
    MIFFT_HALF_ROWS(mifft::TileCfg<double, 240, 3, 8, 6, 5, 1, 8, 256, false, true, false, 2, 1, false, 0, false, false, 1, false, double, false, false, 0, false, false, true>),  // rows480_f64_r2c_8x6x5_ntl
    MIFFT_HALF_ROWS(mifft::TileCfg<double, 240, 3, 8, 6, 5, 1, 8, 256, false, false, true, 2, 1, false, 0, false, false, 0, false, double, false, false, 0, false, false, false, true>),  // rows480_f64_c2r_8x6x5
    MIFFT_HALF_ROWS(mifft::TileCfg<double, 512, 3, 8, 8, 8, 1, 4, 256, false, true, false, 2, 1, false, 0, false, false, 0, false, double, false, false, 0, false, false, true>),  // rows1024_f64_r2c_8x8x8
    MIFFT_HALF_ROWS(mifft::TileCfg<double, 512, 3, 8, 8, 8, 1, 4, 256, false, true, false, 2, 1, false, 0, false, false, 1, false, double, false, false, 0, false, false, true>),  // rows1024_f64_r2c_8x8x8_ntl
    MIFFT_HALF_ROWS(mifft::TileCfg<double, 512, 3, 8, 8, 8, 1, 4, 256, false, false, true, 2, 1, false, 0, false, false, 0, false, double, false, false, 0, false, false, false, true>),  // rows1024_f64_c2r_8x8x8
    MIFFT_HALF_ROWS(mifft::TileCfg<double, 540, 3, 10, 9, 6, 1, 3, 256, false, true, false, 2, 1, false, 0, false, false, 0, false, double, false, false, 0, false, false, true>),  // rows1080_f64_r2c_10x9x6
    MIFFT_HALF_ROWS(mifft::TileCfg<double, 540, 3, 10, 9, 6, 1, 3, 256, false, true, false, 2, 1, false, 0, false, false, 1, false, double, false, false, 0, false, false, true>),  // rows1080_f64_r2c_10x9x6_ntl
    MIFFT_HALF_ROWS(mifft::TileCfg<double, 540, 3, 10, 9, 6, 1, 3, 256, false, false, true, 2, 1, false, 0, false, false, 0, false, double, false, false, 0, false, false, false, true>),  // rows1080_f64_c2r_10x9x6
    MIFFT_HALF_ROWS(mifft::TileCfg<double, 960, 4, 8, 6, 5, 4, 2, 256, false, true, false, 2, 1, false, 0, false, false, 0, false, double, false, false, 0, false, false, true>),  // rows1920_f64_r2c_8x6x5x4
    MIFFT_HALF_ROWS(mifft::TileCfg<double, 960, 4, 8, 6, 5, 4, 2, 256, false, true, false, 2, 1, false, 0, false, false, 1, false, double, false, false, 0, false, false, true>),  // rows1920_f64_r2c_8x6x5x4_ntl
    MIFFT_HALF_ROWS(mifft::TileCfg<double, 960, 4, 8, 6, 5, 4, 2, 256, false, false, true, 2, 1, false, 0, false, false, 0, false, double, false, false, 0, false, false, false, true>),  // rows1920_f64_c2r_8x6x5x4
};

const HalfRowsKernel* half_rows_kernels(int* count) {
    *count = (int)(sizeof kHalfRows / sizeof kHalfRows[0]);
    return kHalfRows;
}

}  // namespace mifft
