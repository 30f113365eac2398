// In-place column swap (k_copy with swap = 1, the vector part of swap_columns, qr.fypp:192-194) against the reference's three copies
// through a spare column, on the SHIPPED kernel with the engine's launch rule (blas1_grid: 2 blocks of 256 threads per CU; non-temporal
// from 32 MB columns on).  Both sides interleaved round by round in one process, each round timed by device events around `reps` calls;
// the result of either side is checked against the exchanged inputs first.
//   hipcc --offload-arch=gfx950 -O3 -o tools/swap_probe tools/swap_probe.hip && tools/swap_probe [rounds] [reps] > profiles/swap_columns.txt
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../lightkrylov_amd/csrc/lk_kernels.hip.h"
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

static int grid_for(int num_cu, int64_t nd) {
    int64_t g = (nd / 2 + 1 + 255) / 256, cap = (int64_t)num_cu * 2;
    return (int)std::max<int64_t>(1, std::min(g, cap));
}

int main(int argc, char **argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 9, reps = argc > 2 ? atoi(argv[2]) : 20;
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int num_cu = prop.multiProcessorCount;
    printf("# k_copy swap = 1 against three k_copy calls through a spare column; real kind; %s, %d CUs; %d rounds x %d calls, interleaved\n",
           prop.name, num_cu, rounds, reps);
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    for (int64_t n : {(int64_t)10000000, (int64_t)100000000}) {
        const int64_t ld = n + 32;                       // columns 256-byte aligned, as in an engine panel
        double *d = nullptr;
        CK(hipMalloc(&d, (size_t)3 * ld * sizeof(double)));
        double *x = d, *y = d + ld, *t = d + 2 * ld;
        std::vector<double> hx(n), hy(n), back(n);
        for (int64_t i = 0; i < n; ++i) { hx[i] = 1.0 + (double)(i % 1009); hy[i] = -2.0 - (double)(i % 997); }
        CK(hipMemcpy(x, hx.data(), n * sizeof(double), hipMemcpyHostToDevice));
        CK(hipMemcpy(y, hy.data(), n * sizeof(double), hipMemcpyHostToDevice));
        const int g = grid_for(num_cu, n), nt = n * 8 >= ((int64_t)32 << 20);
        auto swap = [&]() { hipLaunchKernelGGL(lk::k_copy, dim3(g), dim3(256), 0, 0, x, y, n, nt, 1); };
        auto copies = [&]() {
            hipLaunchKernelGGL(lk::k_copy, dim3(g), dim3(256), 0, 0, y, t, n, nt, 0);     // copy(Qwrk, Q(j))
            hipLaunchKernelGGL(lk::k_copy, dim3(g), dim3(256), 0, 0, x, y, n, nt, 0);     // copy(Q(j), Q(i))
            hipLaunchKernelGGL(lk::k_copy, dim3(g), dim3(256), 0, 0, t, x, n, nt, 0);     // copy(Q(i), Qwrk)
        };
        // one call of each: x and y exchanged, then exchanged back
        swap();
        CK(hipMemcpy(back.data(), x, n * sizeof(double), hipMemcpyDeviceToHost));
        if (back != hy) { printf("swap: x is not the old y\n"); return 2; }
        CK(hipMemcpy(back.data(), y, n * sizeof(double), hipMemcpyDeviceToHost));
        if (back != hx) { printf("swap: y is not the old x\n"); return 2; }
        copies();
        CK(hipMemcpy(back.data(), x, n * sizeof(double), hipMemcpyDeviceToHost));
        if (back != hx) { printf("three copies: x is not restored\n"); return 2; }
        std::vector<float> ms_swap, ms_copy;
        for (int r = 0; r < rounds + 1; ++r) {           // round 0 is the warm-up
            float a = 0.f, b = 0.f;
            CK(hipEventRecord(e0, 0));
            for (int i = 0; i < reps; ++i) swap();
            CK(hipEventRecord(e1, 0));
            CK(hipEventSynchronize(e1));
            CK(hipEventElapsedTime(&a, e0, e1));
            CK(hipEventRecord(e0, 0));
            for (int i = 0; i < reps; ++i) copies();
            CK(hipEventRecord(e1, 0));
            CK(hipEventSynchronize(e1));
            CK(hipEventElapsedTime(&b, e0, e1));
            if (r) { ms_swap.push_back(a / reps); ms_copy.push_back(b / reps); }
        }
        std::sort(ms_swap.begin(), ms_swap.end());
        std::sort(ms_copy.begin(), ms_copy.end());
        const float s = ms_swap[ms_swap.size() / 2], c3 = ms_copy[ms_copy.size() / 2];
        printf("n = %lld (nt = %d, grid %d): swap %.4f ms (min %.4f max %.4f; %.0f GB/s on 32 B per element) | three copies %.4f ms (min %.4f max %.4f; "
               "%.0f GB/s on 48 B per element) | swap / three copies = %.3f\n",
               (long long)n, nt, g, s, ms_swap.front(), ms_swap.back(), 32.0 * n / s * 1e-6, c3, ms_copy.front(), ms_copy.back(),
               48.0 * n / c3 * 1e-6, s / c3);
        CK(hipFree(d));
    }
    return 0;
}
