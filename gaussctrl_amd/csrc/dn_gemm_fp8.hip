// dn_gemm_fp8.hip -- instantiates k_gemm8q: OCP fp8 (e4m3) operands on the block-scaled MFMA (BASELINE configs[3]).
#include "dn_gemm_kernels.h"

namespace {
template <class T, int MODE, int NTW, int MT>
void launch8q(const GemmArgs &g, dim3 grid, hipStream_t s)
{
    constexpr size_t lds = 3 * (64 * MT * 128 + 32 * NTW * 128) + 64 * MT * 8;
    static_assert(lds <= 160 * 1024, "LDS ring");
    static gc::AttrOnce once[2];
    if (fuse_of(g)) {
        gc::ensure_dynamic_lds(once[1], (const void *)k_gemm8q<T, MODE, NTW, MT, true>, (int)lds);
        hipLaunchKernelGGL((k_gemm8q<T, MODE, NTW, MT, true>), grid, dim3(512), lds, s, g);
    } else {
        gc::ensure_dynamic_lds(once[0], (const void *)k_gemm8q<T, MODE, NTW, MT, false>, (int)lds);
        hipLaunchKernelGGL((k_gemm8q<T, MODE, NTW, MT, false>), grid, dim3(512), lds, s, g);
    }
}
// channel-partial epilogue (GemmArgs::chan_parts): fast convs whose output feeds a GroupNorm
template <class T, int NTW, int MT>
void launch8q_cs(const GemmArgs &g, dim3 grid, hipStream_t s)
{
    constexpr size_t lds = 3 * (64 * MT * 128 + 32 * NTW * 128) + 32 * NTW * 16;
    static_assert(lds <= 160 * 1024, "LDS ring");
    static gc::AttrOnce once;
    gc::ensure_dynamic_lds(once, (const void *)k_gemm8q<T, 2, NTW, MT, false, true>, (int)lds);
    hipLaunchKernelGGL((k_gemm8q<T, 2, NTW, MT, false, true>), grid, dim3(512), lds, s, g);
}
template <class T>
void dispatch8q(const GemmArgs &g, int mode, int ntw, int mt, dim3 grid, hipStream_t s)
{
    // the wave tiles that fit under 256 VGPRs, and no others instantiated: (5, 2) (4, 2) (4, 3)
    if (ntw == 5 || mt != 3) mt = 2;
    with_wave_tile(ntw, mt, [&](auto ntw_, auto mt_) {
        constexpr int NTW = decltype(ntw_)::value, MT = decltype(mt_)::value;
        if constexpr (MT == 2 || (NTW == 4 && MT == 3)) {
            if (g.chan_parts && g.splits == 1) launch8q_cs<T, NTW, MT>(g, grid, s);      // (the launcher admits this for mode 2 without fused statistics only)
            else if (mode == 2) launch8q<T, 2, NTW, MT>(g, grid, s);
            else launch8q<T, 3, NTW, MT>(g, grid, s);
        }
    });
}
}  // namespace

void dn_gemm_launch_fp8(const GemmArgs &g, int dtype, int mode, int ntw, int mt, dim3 grid, hipStream_t s)
{
    if (dtype == DT_BF16) dispatch8q<BF16>(g, mode, ntw, mt, grid, s); else dispatch8q<F16>(g, mode, ntw, mt, grid, s);
}
