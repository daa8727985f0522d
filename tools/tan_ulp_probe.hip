// The largest difference, in ulps of the host's result, between the device's tan(double) and the host's std::tan over a
// dense sweep of [1e-8, 2.0]: the bound behind k_undistort_fisheye's guard band (csrc/undistort.hip).
//   hipcc --offload-arch=gfx950 -O2 -ffp-contract=off -o tan_ulp_probe tools/tan_ulp_probe.hip
//   ./tan_ulp_probe [points per sweep, default 2^24] [out.json]
// Three sweeps: logarithmic over [1e-8, 2], linear over [0, 2], and linear over [pi/2 - 2^-10, pi/2 + 2^-10] (the
// reference's own calibration ends its iteration past the pole).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <cmath>
#include <vector>

__global__ void k_tan(const double* __restrict__ x, int n, double* __restrict__ y) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = tan(x[i]);
}

static int64_t ordered(double v) {   // a monotone integer image of the doubles: adjacent doubles differ by 1
    int64_t b;
    memcpy(&b, &v, 8);
    return b < 0 ? INT64_MIN - b : b;
}

#define CHECK(call)                                                            \
    do {                                                                       \
        hipError_t e_ = (call);                                                \
        if (e_ != hipSuccess) {                                                \
            fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_));         \
            return 1;                                                          \
        }                                                                      \
    } while (0)

int main(int argc, char** argv) {
    const int n = argc > 1 ? atoi(argv[1]) : 1 << 24;
    if (n < 2) return 2;
    const double half_pi = 3.1415926535897932384626433832795 / 2.0;
    std::vector<double> x((size_t)n), y((size_t)n);
    double *d_x = nullptr, *d_y = nullptr;
    CHECK(hipMalloc((void**)&d_x, (size_t)n * 8));
    CHECK(hipMalloc((void**)&d_y, (size_t)n * 8));
    long long worst[3] = {0, 0, 0};
    double worst_x[3] = {0, 0, 0};
    for (int sweep = 0; sweep < 3; sweep++) {
        for (int i = 0; i < n; i++) {
            const double t = (double)i / (double)(n - 1);
            x[i] = sweep == 0 ? 1e-8 * std::exp(t * std::log(2.0 / 1e-8))
                 : sweep == 1 ? 1e-8 + t * (2.0 - 1e-8)
                              : half_pi + (2.0 * t - 1.0) * 0x1p-10;
        }
        CHECK(hipMemcpy(d_x, x.data(), (size_t)n * 8, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_tan, dim3((n + 255) / 256), dim3(256), 0, 0, d_x, n, d_y);
        CHECK(hipGetLastError());
        CHECK(hipMemcpy(y.data(), d_y, (size_t)n * 8, hipMemcpyDeviceToHost));
        for (int i = 0; i < n; i++) {
            const double h = std::tan(x[i]);
            long long d = ordered(y[i]) - ordered(h);
            if (d < 0) d = -d;
            if (d > worst[sweep]) {
                worst[sweep] = d;
                worst_x[sweep] = x[i];
            }
        }
    }
    char line[512];
    snprintf(line, sizeof line,
             "{\"points_per_sweep\": %d, \"max_ulp_log\": %lld, \"at_log\": %.17g, \"max_ulp_linear\": %lld, "
             "\"at_linear\": %.17g, \"max_ulp_pole\": %lld, \"at_pole\": %.17g}\n",
             n, worst[0], worst_x[0], worst[1], worst_x[1], worst[2], worst_x[2]);
    fputs(line, stdout);
    if (argc > 2) {
        FILE* f = fopen(argv[2], "w");
        if (!f) return 1;
        fputs(line, f);
        fclose(f);
    }
    (void)hipFree(d_x);
    (void)hipFree(d_y);
    return 0;
}
