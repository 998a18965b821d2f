// resolve_vs_copy.hip -- measurement (not product): the fold kernel of a supersampled launch (rtx_resolve, csrc/rtx_resolve_kernels.inc)
// alone, against a device-to-device hipMemcpyAsync of the same number of input bytes, in ONE process, the two alternating round by
// round.  The copy is the yardstick: the fold reads 32 S^2 bytes per cell once and writes 4 .. 32, the copy reads and writes them.
//
// This file compiles the library's own kernel text (it includes csrc/rtx_kernels.hip) and launches through its launch function, so
// what is timed is the instantiation the library runs.  tools/supersample_cost_gpu.py builds nothing: build here first,
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -fno-slp-vectorize -Wno-unused-function -Wno-unused-value
//         -Wno-unused-result -Wno-pass-failed -o resolve_vs_copy resolve_vs_copy.hip      (add -DRTX_RESOLVE_NT_LOADS for the A/B of the loads)
// and run   ./resolve_vs_copy W H S [rounds] [launches per round]
// which prints one line: the case, the bytes, and for the fold in its three output forms and for the copy the median [min-max] over
// the rounds of the time per launch in us (device events around `launches` launches queued back to back on one stream).
#include "../../raytracing-in-windows-console_amd/csrc/rtx_kernels.hip"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(call)                                                                                   \
    do {                                                                                           \
        hipError_t e__ = (call);                                                                   \
        if (e__ != hipSuccess) {                                                                   \
            std::fprintf(stderr, "%s: %s (line %d)\n", #call, hipGetErrorString(e__), __LINE__);   \
            return 1;                                                                              \
        }                                                                                          \
    } while (0)

// Samples as a frame has them: runs of visible samples (distance below far) and of misses, values in the ranges of a shaded pixel.
__global__ void fill_samples(float4* s, size_t n, uint32_t sample_w)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t col = (uint32_t)(i % sample_w), row = (uint32_t)(i / sample_w);
        uint32_t h = (col >> 4) * 2654435761u ^ (row >> 4) * 2246822519u;
        h ^= h >> 15;
        const bool hit = (h & 3u) != 0u;
        const float u = (float)((col * 7u + row * 13u) & 255u) / 255.0f;
        s[2 * i] = hit ? make_float4(10.0f + 20.0f * u, u, 0.6f, 0.8f * u) : make_float4(99999999.f, 0.0f, 0.0f, 0.0f);
        s[2 * i + 1] = hit ? make_float4(0.3f, 255.0f * u, 128.0f, 31.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

static void summary(std::vector<float>& us, char* out, size_t n)
{
    std::sort(us.begin(), us.end());
    std::snprintf(out, n, "%.2f [%.2f-%.2f]", us[us.size() / 2], us.front(), us.back());
}

int main(int argc, char** argv)
{
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s W H S [rounds] [launches per round]\n", argv[0]);
        return 2;
    }
    const uint32_t W = (uint32_t)std::atoi(argv[1]), H = (uint32_t)std::atoi(argv[2]);
    const int S = std::atoi(argv[3]), rounds = argc > 4 ? std::atoi(argv[4]) : 9;
    int launches = argc > 5 ? std::atoi(argv[5]) : 0;
    const rtxplan::SamplePlan sp = rtxplan::plan_supersample(W, H, 0, H, S);
    if (!sp.ok || S < 2 || rounds < 1) {
        std::fprintf(stderr, "refused: W, H in [1, 2^31 / S), S in 2 .. 4\n");
        return 2;
    }
    const size_t in_bytes = (size_t)sp.bytes, n_samples = (size_t)(sp.W * sp.rows);
    if (launches <= 0) launches = (int)std::max<size_t>(20, std::min<size_t>(2000, ((size_t)2 << 30) / in_bytes)); // about 2 GB of input a round
    float4 *samples = nullptr, *copy_dst = nullptr;
    uint8_t *out = nullptr, *grey = nullptr;
    hipStream_t st;
    hipEvent_t e0, e1;
    CK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    CK(hipMalloc(&samples, in_bytes));
    CK(hipMalloc(&copy_dst, in_bytes));
    CK(hipMalloc(&out, (size_t)32 * W * H));
    CK(hipMalloc(&grey, 256));
    CK(hipMemset(grey, 0, 256));
    hipLaunchKernelGGL(fill_samples, dim3(2048), dim3(256), 0, st, samples, n_samples, (uint32_t)sp.W);
    CK(hipGetLastError());
    CK(hipStreamSynchronize(st));

    KArgs a;
    std::memset(&a, 0, sizeof a);
    a.far = 250.0f;
    a.W = W;
    a.H = H;
    a.row0 = 0;
    a.row_end = H;
    a.out = out;
    a.grey = grey;
    const int kForms = 3;
    const char* form_name[kForms] = {"records", "words", "values"};
    std::vector<float> us[kForms + 1];
    const char* kernel[kForms] = {"", "", ""};
    for (int r = -1; r < rounds; r++) { // (round -1 warms every launch up and is not kept)
        for (int f = 0; f <= kForms; f++) {
            a.compact = (uint32_t)f;
            CK(hipEventRecord(e0, st));
            for (int i = 0; i < launches; i++) {
                if (f == kForms) {
                    CK(hipMemcpyAsync(copy_dst, samples, in_bytes, hipMemcpyDeviceToDevice, st));
                } else {
                    int herr = 0;
                    const char* name = rtx_k_launch_resolve(&a, samples, S, RTX_K_RGB_ASCII, st, &herr);
                    if (!name || herr != 0) {
                        std::fprintf(stderr, "fold launch refused or failed (%d)\n", herr);
                        return 1;
                    }
                    kernel[f] = name;
                }
            }
            CK(hipEventRecord(e1, st));
            CK(hipEventSynchronize(e1));
            float ms = 0.0f;
            CK(hipEventElapsedTime(&ms, e0, e1));
            if (r >= 0) us[f].push_back(1e3f * ms / (float)launches);
        }
    }
    char text[kForms + 1][64];
    for (int f = 0; f <= kForms; f++) summary(us[f], text[f], sizeof text[f]);
    const float copy_med = us[kForms][us[kForms].size() / 2];
    std::printf("fold alone, %u x %u cells, S = %d: %.1f MB in | us per launch, median [min-max] over %d rounds of %d launches", W, H, S, (double)in_bytes / 1e6, rounds, launches);
    for (int f = 0; f < kForms; f++) {
        std::printf(" | %s %s (%.2f x copy, %.0f GB/s in) %s", form_name[f], text[f], us[f][us[f].size() / 2] / copy_med, (double)in_bytes / 1e3 / us[f][us[f].size() / 2], kernel[f]);
    }
    std::printf(" | hipMemcpyAsync D2D of the same bytes %s (%.0f GB/s in)\n", text[kForms], (double)in_bytes / 1e3 / copy_med);
    hipFree(samples);
    hipFree(copy_dst);
    hipFree(out);
    hipFree(grey);
    return 0;
}
