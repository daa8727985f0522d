// What buffer_load_format_d16_xyzw returns on gfx950 through a raw (stride 0) descriptor with DATA_FORMAT 8_8_8_8,
// NUM_FORMAT UINT and identity DST_SEL, and what it costs against buffer_load_dword: k_fast_wave widens the u8 ROI
// to the u16 pixel pairs of its LDS tile, which is what this load's format conversion produces ((b0, b1), (b2, b3)
// as two VGPRs) in the memory pipeline.
//   (a) voffset = 4 * lane: b0 | b1 << 16, b2 | b3 << 16 for every lane; an offset past num_records and the
//       0x40000000 offset of fast_roi_issue's idle lanes read 0
//   (b) voffset = 1, 2, 3 (mod 4): the four bytes from that offset, the dword rounded down, or something else;
//       and a load that straddles num_records
//   (c) time of 8 independent loads per lane and one wait, format against dword, aligned and 3 (mod 4)
//   make -C orb-slam-birdview_amd ../tools/format_load_probe && tools/format_load_probe
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <vector>

typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
// the raw-buffer format load of four 16-bit components: selects buffer_load_format_d16_xyzw, and the compiler
// tracks its vmcnt like any other load
__device__ half4_t raw_buffer_load_format_d16x4(__amdgpu_buffer_rsrc_t rsrc, int voffset, int soffset, int aux)
    __asm("llvm.amdgcn.raw.ptr.buffer.load.format.v4f16");

// descriptor word 3: DST_SEL x, y, z, w = 4, 5, 6, 7 (bits 0..11), NUM_FORMAT UINT = 4 (bits 12..14), DATA_FORMAT
// 8_8_8_8 = 10 (bits 15..18); a plain dword load ignores all three
constexpr int kRsrcU8x4 = 0xFAC | (4 << 12) | (10 << 15);

#define CHECK(x)                                                                  \
    do {                                                                          \
        hipError_t e_ = (x);                                                      \
        if (e_ != hipSuccess) {                                                   \
            printf("%s: %s\n", #x, hipGetErrorString(e_));                        \
            return 2;                                                             \
        }                                                                         \
    } while (0)

__global__ void k_values(const uint8_t* p, int num_records, int lane_step, int offset0, u32x2_t* out) {
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(p), 0, num_records, kRsrcU8x4);
    const int off = offset0 + lane_step * (int)threadIdx.x;
    out[threadIdx.x] = __builtin_bit_cast(u32x2_t, raw_buffer_load_format_d16x4(rsrc, off, 0, 0));
}

// 8 independent loads per lane (rows `pitch` bytes apart, as fast_roi_issue's rounds), one wait, `iters` times over
// an L2-resident buffer of `bytes` (a power of two)
template <bool FMT>
__global__ void k_rate(const uint8_t* p, int bytes, int pitch, int mis, int iters, uint32_t* out) {
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(p), 0, bytes, kRsrcU8x4);
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t acc = 0;
    for (int i = 0; i < iters; i++) {
        const int off = (((t + i * 4099) * 4) & (bytes - 1 - 8 * pitch)) + mis;
        if (FMT) {
            u32x2_t v[8];
#pragma unroll
            for (int k = 0; k < 8; k++) v[k] = __builtin_bit_cast(u32x2_t, raw_buffer_load_format_d16x4(rsrc, off + k * pitch, 0, 0));
#pragma unroll
            for (int k = 0; k < 8; k++) acc += v[k].x ^ v[k].y;
        } else {
            uint32_t v[8];
#pragma unroll
            for (int k = 0; k < 8; k++) v[k] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, off + k * pitch, 0, 0);
#pragma unroll
            for (int k = 0; k < 8; k++) acc += v[k];
        }
    }
    out[t] = acc;
}

static uint8_t ramp(long long i) { return (uint8_t)(i * 7 + 3); }

int main() {
    const int N = 1 << 20;
    std::vector<uint8_t> h(N);
    for (int i = 0; i < N; i++) h[i] = ramp(i);
    uint8_t* d;
    u32x2_t* dout;
    CHECK(hipMalloc(&d, N));
    CHECK(hipMalloc(&dout, 64 * sizeof(u32x2_t)));
    CHECK(hipMemcpy(d, h.data(), N, hipMemcpyHostToDevice));
    u32x2_t r[64];
    auto run = [&](int num_records, int step, int off0) {
        hipLaunchKernelGGL(k_values, dim3(1), dim3(64), 0, 0, d, num_records, step, off0, dout);
        return hipMemcpy(r, dout, sizeof r, hipMemcpyDeviceToHost);
    };
    auto pair = [&](long long o, int j) { return (uint32_t)ramp(o + 2 * j) | (uint32_t)ramp(o + 2 * j + 1) << 16; };

    // (a) aligned offsets, all in range; then lanes from 32 on past num_records; then the 0x40000000 offset
    int bad = 0;
    CHECK(run(4096, 4, 0));
    for (int l = 0; l < 64; l++) bad += r[l].x != pair(4 * l, 0) || r[l].y != pair(4 * l, 1);
    printf("(a) aligned, in range: lane 0 %08x %08x, lane 63 %08x %08x, %d of 64 lanes differ from (b0|b1<<16, b2|b3<<16)\n",
           r[0].x, r[0].y, r[63].x, r[63].y, bad);
    int bad_oor = 0;
    CHECK(run(128, 4, 0));
    for (int l = 0; l < 64; l++)
        bad_oor += l < 32 ? (r[l].x != pair(4 * l, 0) || r[l].y != pair(4 * l, 1)) : (r[l].x != 0 || r[l].y != 0);
    printf("(a) num_records 128: lane 31 %08x %08x, lane 32 %08x %08x, %d lanes wrong (in range: data, past: 0)\n",
           r[31].x, r[31].y, r[32].x, r[32].y, bad_oor);
    int bad_big = 0;
    CHECK(run(4096, 4, 0x40000000));
    for (int l = 0; l < 64; l++) bad_big += r[l].x != 0 || r[l].y != 0;
    printf("(a) voffset 0x40000000 + 4 lane: %d lanes not 0\n", bad_big);
    const bool a_ok = !bad && !bad_oor && !bad_big;
    printf("(a) %s\n", a_ok ? "PASS" : "FAIL");

    // (b) offsets 1, 2, 3 (mod 4)
    for (int m = 1; m < 4; m++) {
        CHECK(run(4096, 4, m));
        int exact = 0, down = 0;
        for (int l = 0; l < 64; l++) {
            exact += r[l].x == pair(4 * l + m, 0) && r[l].y == pair(4 * l + m, 1);
            down += r[l].x == pair(4 * l, 0) && r[l].y == pair(4 * l, 1);
        }
        printf("(b) voffset = %d (mod 4): lane 0 %08x %08x (bytes from the offset: %08x %08x; dword rounded down: %08x %08x): "
               "%d lanes byte-exact, %d lanes rounded down\n",
               m, r[0].x, r[0].y, pair(m, 0), pair(m, 1), pair(0, 0), pair(0, 1), exact, down);
    }
    // a descriptor whose base is odd (the even form would move the base one byte down), aligned voffsets
    {
        hipLaunchKernelGGL(k_values, dim3(1), dim3(64), 0, 0, d + 3, 4096, 4, 0, dout);
        CHECK(hipMemcpy(r, dout, sizeof r, hipMemcpyDeviceToHost));
        int exact = 0;
        for (int l = 0; l < 64; l++) exact += r[l].x == pair(4 * l + 3, 0) && r[l].y == pair(4 * l + 3, 1);
        printf("(b) base + 3, voffset 4 lane: lane 0 %08x %08x (bytes from base + 3: %08x %08x): %d lanes byte-exact\n", r[0].x,
               r[0].y, pair(3, 0), pair(3, 1), exact);
    }
    // loads that straddle num_records (126: lane 31's bytes 124..127 are half in range)
    CHECK(run(126, 4, 0));
    printf("(b) num_records 126: lane 30 %08x %08x, lane 31 (bytes 124..127) %08x %08x (all in range would be %08x %08x)\n",
           r[30].x, r[30].y, r[31].x, r[31].y, pair(124, 0), pair(124, 1));
    CHECK(run(127, 4, 3));
    printf("(b) num_records 127, voffset 4 lane + 3: lane 30 (bytes 123..126) %08x %08x (bytes: %08x %08x), lane 31 (127..130) %08x %08x\n",
           r[30].x, r[30].y, pair(123, 0), pair(123, 1), r[31].x, r[31].y);

    // (c) rate: 1024 blocks of 256 lanes, 64 rounds of 8 loads per lane
    uint32_t* dacc;
    const int blocks = 1024, threads = 256, iters = 64, pitch = 1280;
    CHECK(hipMalloc(&dacc, blocks * threads * 4));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    auto timeit = [&](bool fmt, int mis) {
        std::vector<float> ms;
        for (int rep = 0; rep < 7; rep++) {
            hipEventRecord(e0, 0);
            if (fmt) hipLaunchKernelGGL(k_rate<true>, dim3(blocks), dim3(threads), 0, 0, d, N, pitch, mis, iters, dacc);
            else hipLaunchKernelGGL(k_rate<false>, dim3(blocks), dim3(threads), 0, 0, d, N, pitch, mis, iters, dacc);
            hipEventRecord(e1, 0);
            hipEventSynchronize(e1);
            float t = 0;
            hipEventElapsedTime(&t, e0, e1);
            if (rep >= 2) ms.push_back(t);   // two warm-up launches
        }
        std::sort(ms.begin(), ms.end());
        return ms[ms.size() / 2];
    };
    const float t_dw = timeit(false, 0), t_fmt = timeit(true, 0), t_dw3 = timeit(false, 3), t_fmt3 = timeit(true, 3);
    CHECK(hipDeviceSynchronize());
    const double loads = (double)blocks * threads / 64 * iters * 8;
    printf("(c) %.0f wave loads per launch, median of 5: dword %.4f ms (%.2f G wave loads/s), format_d16_xyzw %.4f ms (%.2f G/s), "
           "ratio %.2f\n", loads, t_dw, loads / t_dw * 1e-6, t_fmt, loads / t_fmt * 1e-6, t_fmt / t_dw);
    printf("(c) voffset = 3 (mod 4): dword %.4f ms, format_d16_xyzw %.4f ms, ratio to the aligned dword %.2f\n", t_dw3, t_fmt3,
           t_fmt3 / t_dw);
    return a_ok ? 0 : 1;
}
