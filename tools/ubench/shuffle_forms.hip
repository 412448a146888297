// Micro-benchmark: two forms of the pixel-shuffle kernel (csrc/shuffle.hip) at ResShuffleDecoder's two shapes with 512 frames,
// ReLU applied, no max |.| record.  "scalar": a thread owns one channel of a coarse pixel (one float4 load, four scalar stores);
// "quad": a thread owns four channels, transposes 4 x 4 in registers and stores four float4.  Three rounds of 50 back-to-back
// launches each, the forms alternating; the two outputs are compared element by element.  DESIGN 3.10 quotes the result.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/ubench/shuffle_forms.hip -o tools/ubench/shuffle_forms && tools/ubench/shuffle_forms
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(1); } } while (0)
#define T 256
__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ void st4(float *p, float4 v) { *reinterpret_cast<float4 *>(p) = v; }

// form A: a thread owns one coarse float4 (one channel, four sub-pixels) and stores four scalars
__global__ __launch_bounds__(T) void form_scalar(const float *__restrict__ x, long long n, int Cp, int W, int C, float *__restrict__ out) {
    const long long rowf = 2LL * W * Cp;
    for (long long i = (long long)blockIdx.x * T + threadIdx.x; i < n; i += (long long)gridDim.x * T) {
        const long long pix = i / Cp;
        const int c = (int)(i - pix * Cp);
        const long long r = pix / W;
        const int j = (int)(pix - r * W);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < C) { v = ld4(x + (pix * C + c) * 4); v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
        const long long o = 2 * r * rowf + (long long)2 * j * Cp + c;
        out[o] = v.x; out[o + Cp] = v.y; out[o + rowf] = v.z; out[o + rowf + Cp] = v.w;
    }
}
// form B: a thread owns four channels of a coarse pixel, transposes 4 x 4 in registers, stores four float4
__global__ __launch_bounds__(T) void form_quad(const float *__restrict__ x, long long n4, int q, int W, int C, float *__restrict__ out) {
    const long long rowf = 2LL * W * q * 4;
    for (long long i = (long long)blockIdx.x * T + threadIdx.x; i < n4; i += (long long)gridDim.x * T) {
        const long long pix = i / q;
        const int c4 = (int)(i - pix * q);
        const long long r = pix / W;
        const int j = (int)(pix - r * W);
        const int nr = C - 4 * c4;
        const float *p = x + (pix * C + 4 * c4) * 4;
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        float4 a = ld4(p), b = nr > 1 ? ld4(p + 4) : z, c = nr > 2 ? ld4(p + 8) : z, d = nr > 3 ? ld4(p + 12) : z;
        const long long o = 2 * r * rowf + ((long long)2 * j * q + c4) * 4;
        st4(out + o, make_float4(fmaxf(a.x, 0.f), fmaxf(b.x, 0.f), fmaxf(c.x, 0.f), fmaxf(d.x, 0.f)));
        st4(out + o + 4 * q, make_float4(fmaxf(a.y, 0.f), fmaxf(b.y, 0.f), fmaxf(c.y, 0.f), fmaxf(d.y, 0.f)));
        st4(out + o + rowf, make_float4(fmaxf(a.z, 0.f), fmaxf(b.z, 0.f), fmaxf(c.z, 0.f), fmaxf(d.z, 0.f)));
        st4(out + o + rowf + 4 * q, make_float4(fmaxf(a.w, 0.f), fmaxf(b.w, 0.f), fmaxf(c.w, 0.f), fmaxf(d.w, 0.f)));
    }
}
static unsigned grid_for(long long n) { long long b = (n + T - 1) / T; return (unsigned)(b < 2048 ? b : 2048); }

int main() {
    const int shapes[2][4] = {{512, 16, 16, 128}, {512, 32, 32, 3}};
    for (int s = 0; s < 2; ++s) {
        const int N = shapes[s][0], H = shapes[s][1], W = shapes[s][2], C = shapes[s][3], Cp = (C + 3) / 4 * 4, q = Cp / 4;
        const long long nin = (long long)N * H * W * 4 * C, nout = (long long)N * 4 * H * W * Cp;
        float *x, *oa, *ob;
        CK(hipMalloc(&x, nin * 4)); CK(hipMalloc(&oa, nout * 4)); CK(hipMalloc(&ob, nout * 4));
        std::vector<float> h(nin);
        for (long long i = 0; i < nin; ++i) h[i] = (float)((i * 2654435761u) % 2001) / 1000.f - 1.f;
        CK(hipMemcpy(x, h.data(), nin * 4, hipMemcpyHostToDevice));
        const long long na = (long long)N * H * W * Cp, nb = (long long)N * H * W * q;
        hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
        for (int round = 0; round < 3; ++round) {
            for (int form = 0; form < 2; ++form) {
                for (int rep = -5; rep < 50; ++rep) {
                    if (rep == 0) CK(hipEventRecord(e0));
                    if (form == 0) form_scalar<<<grid_for(na), T>>>(x, na, Cp, W, C, oa);
                    else form_quad<<<grid_for(nb), T>>>(x, nb, q, W, C, ob);
                }
                CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); CK(hipGetLastError());
                float ms; CK(hipEventElapsedTime(&ms, e0, e1)); ms /= 50;
                printf("shape %dx%dx%dx%d round %d form %s: %.2f us, %.1f GB/s\n", N, H, W, 4 * C, round, form ? "quad" : "scalar", ms * 1e3,
                       (nin + nout) * 4 / ms / 1e6);
            }
        }
        std::vector<float> ra(nout), rb(nout);
        CK(hipMemcpy(ra.data(), oa, nout * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(rb.data(), ob, nout * 4, hipMemcpyDeviceToHost));
        long long bad = 0;
        for (long long i = 0; i < nout; ++i) bad += ra[i] != rb[i];
        printf("shape %d: forms differ in %lld elements\n", s, bad);
        CK(hipFree(x)); CK(hipFree(oa)); CK(hipFree(ob));
    }
    return 0;
}
