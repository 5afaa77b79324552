// Variants of the split-K reduce kernel side by side (diagnostics only, not
// part of the library): plain against nontemporal slab loads, slab loads in
// batches of 4 or 8, grid caps of 1024 / 2048 / 4096 blocks and the uncapped
// grid, on a 4096^2 fp64 C with 1, 3 and 7 slabs (S = 2, 4, 8 without
// accumulation), and an elementwise add (map_kernel's loop) on the same
// byte count. hipEvent time per launch, one warm-up and five repetitions
// per variant, each variant measured in two rounds; prints the
// reduce-variants lines of profiles/gemm_splitk_raw.jsonl. What kernels.hip's
// splitk_reduce_kernel uses (nontemporal, batches of 8, cap 4096) was
// chosen from this; results in profiles/gemm_splitk.md.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 \
//       tools_dev/splitk_reduce_variants.hip -o splitk_reduce_variants
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <vector>
#include <algorithm>

typedef double v2d __attribute__((ext_vector_type(2)));
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s line %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

template <int NT, int BATCH>
__global__ void __launch_bounds__(256)
reduce_k(double* __restrict__ C, int64_t ldc, int64_t m, int64_t n,
         const double* __restrict__ W, int64_t slab, int nslabs) {
    using V = v2d;
    const int64_t per_col = m / 2, total = per_col * n, slab_v = slab / 2;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t col = i / per_col, r = i - col * per_col;
        V* cp = reinterpret_cast<V*>(C + col * ldc) + r;
        const V* wp = reinterpret_cast<const V*>(W) + i;
        V acc = *cp;
        int j = 0;
        for (; j + BATCH <= nslabs; j += BATCH) {
            V w[BATCH];
            #pragma unroll
            for (int b = 0; b < BATCH; b++)
                w[b] = NT ? __builtin_nontemporal_load(&wp[(j + b) * slab_v]) : wp[(j + b) * slab_v];
            #pragma unroll
            for (int b = 0; b < BATCH; b++) acc = acc + w[b];
        }
        for (; j < nslabs; j++) acc = acc + (NT ? __builtin_nontemporal_load(&wp[j * slab_v]) : wp[j * slab_v]);
        *cp = acc;
    }
}

__global__ void map_add(int64_t n, const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ c) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) c[i] = a[i] + b[i];
}

int main() {
    const int64_t m = 4096, n = 4096, slab = m * n;
    double *C, *W, *X, *Y, *Z;
    const int maxslabs = 7;
    CK(hipMalloc(&C, slab * 8));
    CK(hipMalloc(&W, slab * 8 * maxslabs));
    const int64_t nmap_max = (maxslabs + 2) * slab / 3;
    CK(hipMalloc(&X, nmap_max * 8)); CK(hipMalloc(&Y, nmap_max * 8)); CK(hipMalloc(&Z, nmap_max * 8));
    CK(hipMemset(C, 0, slab * 8)); CK(hipMemset(W, 0, slab * 8 * maxslabs));
    CK(hipMemset(X, 0, nmap_max * 8)); CK(hipMemset(Y, 0, nmap_max * 8));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const int64_t chunks = m / 2 * n;
    const unsigned full = (unsigned)((chunks + 255) / 256);
    struct V { const char* name; int nt, batch; unsigned grid; };
    const V vars[] = {{"base-g2048-b4", 0, 4, 2048}, {"nt-g2048-b4", 1, 4, 2048},
                      {"base-full-b4", 0, 4, full}, {"nt-full-b4", 1, 4, full},
                      {"base-g2048-b8", 0, 8, 2048}, {"base-g4096-b4", 0, 4, 4096},
                      {"base-g1024-b4", 0, 4, 1024}, {"nt-g4096-b8", 1, 8, 4096}};
    // one JSON line per slab count: per variant and round [med, min, max] us
    for (int ns : {1, 3, 7}) {
        printf("{\"group\":\"reduce-variants\",\"slabs\":%d,\"bytes\":%lld,\"med_min_max_us\":{", ns, (long long)((ns + 2) * slab * 8));
        for (const V& v : vars) {
        printf("\"%s\":[", v.name);
        for (int round = 0; round < 2; round++) {
            std::vector<float> ms;
            for (int rep = -1; rep < 5; rep++) {
                CK(hipEventRecord(e0, 0));
                if (v.nt == 0 && v.batch == 4) hipLaunchKernelGGL((reduce_k<0, 4>), dim3(v.grid), dim3(256), 0, 0, C, m, m, n, W, slab, ns);
                else if (v.nt == 1 && v.batch == 4) hipLaunchKernelGGL((reduce_k<1, 4>), dim3(v.grid), dim3(256), 0, 0, C, m, m, n, W, slab, ns);
                else if (v.nt == 0 && v.batch == 8) hipLaunchKernelGGL((reduce_k<0, 8>), dim3(v.grid), dim3(256), 0, 0, C, m, m, n, W, slab, ns);
                else hipLaunchKernelGGL((reduce_k<1, 8>), dim3(v.grid), dim3(256), 0, 0, C, m, m, n, W, slab, ns);
                CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1));
                float t; CK(hipEventElapsedTime(&t, e0, e1));
                if (rep >= 0) ms.push_back(t);
            }
            std::sort(ms.begin(), ms.end());
            printf("%s[%.1f,%.1f,%.1f]", round ? "," : "", ms[2] * 1e3, ms[0] * 1e3, ms[4] * 1e3);
        }
        printf("],");
        }
        const int64_t nmap = (ns + 2) * slab / 3;
        std::vector<float> ms;
        for (int rep = -1; rep < 5; rep++) {
            CK(hipEventRecord(e0, 0));
            hipLaunchKernelGGL(map_add, dim3(2048), dim3(256), 0, 0, nmap, X, Y, Z);
            CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1));
            float t; CK(hipEventElapsedTime(&t, e0, e1));
            if (rep >= 0) ms.push_back(t);
        }
        std::sort(ms.begin(), ms.end());
        printf("\"map_add\":[[%.1f,%.1f,%.1f]]}}\n", ms[2] * 1e3, ms[0] * 1e3, ms[4] * 1e3);
    }
    CK(hipDeviceSynchronize());
    return 0;
}
