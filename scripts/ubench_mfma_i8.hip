// ubench_mfma_i8.hip -- the operand lane maps of v_mfma_i32_16x16x64_i8 on gfx950, established with exact integers and asymmetric
// operands.  1024 products on one wave: product T has A all zero except a 1 in byte (T % 16) of lane (T / 16); B holds,
// in byte jb of lane lb, the number 1 + 16 * (lb >> 4) + jb -- the same in every column, different for every (lane group, byte).  The
// 16 x 16 result then has ONE non-zero row: the row that A's lane feeds, holding in every column the B number of the k position A's
// byte is multiplied with.  A second pass swaps the roles (one B byte, numbered A) for the column that a B lane feeds.
//   hipcc --offload-arch=gfx950 -O2 -o ubench_mfma_i8 scripts/ubench_mfma_i8.hip && ./ubench_mfma_i8
// prints what acquire_mfma relies on and "ok", or the first deviation.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <vector>

typedef int i32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(64) void probe(int *out /* [2][1024][64][4] */)
{
    const int lane = threadIdx.x;
    for (int pass = 0; pass < 2; ++pass)
        for (int t = 0; t < 1024; ++t) {
            int8_t one[16], num[16];
            for (int j = 0; j < 16; ++j) {
                one[j] = (lane == t / 16 && j == t % 16) ? 1 : 0;
                num[j] = (int8_t) (1 + 16 * (lane >> 4) + j);
            }
            i32x4 a, b;
            __builtin_memcpy(&a, pass ? num : one, 16);
            __builtin_memcpy(&b, pass ? one : num, 16);
            const i32x4 d = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, i32x4{0, 0, 0, 0}, 0, 0, 0);
            for (int r = 0; r < 4; ++r) out[((pass * 1024 + t) * 64 + lane) * 4 + r] = d[r];
        }
}

int main()
{
    const size_t n = 2 * 1024 * 64 * 4;
    int *d = nullptr;
    if (hipMalloc(&d, n * sizeof(int)) != hipSuccess) { std::printf("no device\n"); return 1; }
    hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, d);
    std::vector<int> h(n);
    if (hipMemcpy(h.data(), d, n * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) { std::printf("copy failed\n"); return 1; }
    // expected: C/D element (row, col) in register row & 3 of lane col + 16 * (row >> 2); A lane l feeds row l & 15, B lane l column l & 15;
    // byte j of lane group g of A meets byte j of lane group g of B
    for (int pass = 0; pass < 2; ++pass)
        for (int t = 0; t < 1024; ++t) {
            const int l = t / 16, j = t % 16, want = 1 + 16 * (l >> 4) + j;
            for (int lane = 0; lane < 64; ++lane)
                for (int r = 0; r < 4; ++r) {
                    const int row = 4 * (lane >> 4) + r, col = lane & 15;
                    const int v = h[((pass * 1024 + t) * 64 + lane) * 4 + r];
                    const int expect = (pass ? col : row) == (l & 15) ? want : 0;
                    if (v != expect) {
                        std::printf("deviation: pass %d, the 1 in lane %d byte %d: D(row %d, col %d) = %d, expected %d\n", pass, l, j, row, col, v, expect);
                        return 1;
                    }
                }
        }
    std::printf("v_mfma_i32_16x16x64_i8: A lane l feeds row l & 15, B lane l feeds column l & 15; byte j of lane group l >> 4 of A meets byte j of\n"
                "lane group l >> 4 of B (2048 one-hot products against numbered operands); D(row, col) is register row & 3 of lane col + 16 * (row >> 2)\nok\n");
    return 0;
}
