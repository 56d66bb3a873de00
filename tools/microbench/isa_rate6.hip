// Issue rate of v_pk_fmac_f16 in its 32-bit VOP2 encoding against v_pk_add_f16 (VOP3P), the subtract of the
// matrix-pipe box kernel's AD (gfx950, wave64): r - l as (-1.0) * l + r with -1.0 in both halves of an SGPR.
// The method of isa_rate4.hip: 8 independent chains per thread, 8 waves per SIMD, every instruction inline asm,
// SIMD cycles per wave-instruction at the 2.4 GHz nominal clock; v_add_u32 and v_and_b32 are the yardsticks.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>

struct Add {
    static constexpr const char* s = "v_add_u32 (VOP2)";
    __device__ static void run(uint32_t& a, uint32_t x, uint32_t) { asm volatile("v_add_u32 %0, %0, %1" : "+v"(a) : "v"(x)); }
};
struct And {
    static constexpr const char* s = "v_and_b32 (VOP2)";
    __device__ static void run(uint32_t& a, uint32_t x, uint32_t) { asm volatile("v_and_b32 %0, %0, %1" : "+v"(a) : "v"(x)); }
};
struct PkAddH {
    static constexpr const char* s = "v_pk_add_f16 neg (VOP3P)";
    __device__ static void run(uint32_t& a, uint32_t x, uint32_t) {
        asm volatile("v_pk_add_f16 %0, %0, %1 neg_lo:[0,1] neg_hi:[0,1]" : "+v"(a) : "v"(x));
    }
};
struct PkFmacHS {
    static constexpr const char* s = "v_pk_fmac_f16 v, s, v (VOP2)";
    __device__ static void run(uint32_t& a, uint32_t x, uint32_t m1) {
        asm volatile("v_pk_fmac_f16 %0, %1, %2" : "+v"(a) : "s"(m1), "v"(x));
    }
};
struct PkFmacHV {
    static constexpr const char* s = "v_pk_fmac_f16 v, v, v (VOP2)";
    __device__ static void run(uint32_t& a, uint32_t x, uint32_t) {
        asm volatile("v_pk_fmac_f16 %0, %1, %1" : "+v"(a) : "v"(x));
    }
};
// the pair as the kernel would issue it: the subtract, then the AND that clears the sign bits
struct PkAddAnd {
    static constexpr const char* s = "v_pk_add_f16 + v_and_b32";
    __device__ static void run(uint32_t& a, uint32_t x, uint32_t) {
        asm volatile("v_pk_add_f16 %0, %0, %1 neg_lo:[0,1] neg_hi:[0,1]\n\tv_and_b32 %0, 0x7fff7fff, %0" : "+v"(a) : "v"(x));
    }
};
struct PkFmacAnd {
    static constexpr const char* s = "v_pk_fmac_f16 v, s, v + v_and_b32";
    __device__ static void run(uint32_t& a, uint32_t x, uint32_t m1) {
        asm volatile("v_pk_fmac_f16 %0, %1, %2\n\tv_and_b32 %0, 0x7fff7fff, %0" : "+v"(a) : "s"(m1), "v"(x));
    }
};

template <class O>
__global__ __launch_bounds__(256) void thr(const uint32_t* in, uint32_t* out, int iters) {
    uint32_t xs[8], acc[8];
    const uint32_t m1 = __builtin_amdgcn_readfirstlane(in[0]);   // 0xBC00BC00: -1.0 in both halves
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        xs[c] = in[1 + ((threadIdx.x + c) & 7)];
        acc[c] = in[1 + ((threadIdx.x * 3 + c) & 7)];
    }
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int k = 0; k < 8; ++k)
#pragma unroll
            for (int c = 0; c < 8; ++c) O::run(acc[c], xs[(c + k) & 7], m1);
    }
    uint32_t s = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) s += acc[c];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

template <class O> void report(const uint32_t* din, uint32_t* dout, int nops = 1) {
    const int blocks = 256 * 8, iters = 512;
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    thr<O><<<blocks, 256>>>(din, dout, iters);
    (void)hipDeviceSynchronize();
    (void)hipEventRecord(e0);
    for (int r = 0; r < 5; ++r) thr<O><<<blocks, 256>>>(din, dout, iters);
    (void)hipEventRecord(e1);
    (void)hipEventSynchronize(e1);
    float ms;
    (void)hipEventElapsedTime(&ms, e0, e1);
    ms /= 5;
    // per SIMD: 8 waves x iters * 64 instructions (x nops asm instructions each)
    const double cyc = ms * 1e-3 * 2.4e9 / (8.0 * iters * 64 * nops);
    printf("%-36s SIMD cycles per wave-instr: %5.2f\n", O::s, cyc);
}

int main() {
    // staged pixels as the kernel holds them: f16 1024 + v in both halves
    uint32_t h[9] = {0xBC00BC00u, 0x64106403u, 0x64FF6400u, 0x64806440u, 0x64016402u,
                     0x647F6480u, 0x64206410u, 0x64C864FAu, 0x64336455u};
    uint32_t *din, *dout;
    if (hipMalloc(&din, sizeof(h)) != hipSuccess || hipMalloc(&dout, 256 * 8 * 256 * 4) != hipSuccess) return 1;
    (void)hipMemcpy(din, h, sizeof(h), hipMemcpyHostToDevice);
    for (int round = 0; round < 2; ++round) {
        report<Add>(din, dout);
        report<And>(din, dout);
        report<PkAddH>(din, dout);
        report<PkFmacHS>(din, dout);
        report<PkFmacHV>(din, dout);
        report<PkAddAnd>(din, dout, 2);
        report<PkFmacAnd>(din, dout, 2);
    }
    return hipDeviceSynchronize() == hipSuccess ? 0 : 1;
}
