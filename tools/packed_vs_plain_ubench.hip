// Packed f32 (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32) against two plain f32 instructions AT THE PAIR KERNEL'S OCCUPANCY
// (gfx950): tools/valu_ubench.hip gave the issue rate of a wave that is almost alone on its SIMD; pair_cull_kernel runs 8 waves per
// SIMD of 64 VGPRs each, where the question is not how fast one wave issues but how long an instruction holds the pipe.
// Every row is timed with the shader clock (s_memtime) on every SIMD at 1, 2, 4 and 8 resident waves per SIMD and printed as
//     SIMD cycles per PAIR OF RESULTS = median over waves of (clock at the end - clock at the start) / (pairs per wave x waves per SIMD)
// for the packed form (one instruction per pair) and the plain form (two).
// "W waves per SIMD" is NOMINAL for W < 8: CUs x W workgroups of four waves are launched and the dispatcher is trusted to give
// every CU W of them, one wave per SIMD - nothing (no LDS padding, no occupancy limit) keeps two workgroups from sharing a CU
// while another has none, and the median over the waves only hides the outliers.  At W = 8, the column the kernel's decision rests
// on, the grid fills every wave slot of the chip (8 per SIMD), so every SIMD does hold eight.
//   independent streams  eight register pairs, each instruction depends on the one eight places back
//   + rsq                the same with one v_rsq_f32 per eight instructions
//   operand kinds        VGPR pair, SGPR pair, inline constant with op_sel_hi - as pair_cull_kernel uses them
//   chains               keep_x2 and field_twod_x2 themselves (csf_field.h), packed and plain, compiled by hipcc with the library's
//                        flags, so that the dependent pairs carry the s_nop the compiler puts behind them; their transcendentals
//                        are the functions' own (keep: 2 per pass, field: 10).  Results are fed back into the next pass's inputs
//                        (a handful of instructions, the same in both forms).  Once with the receiver in scalar registers, as
//                        the packed kernel held it, once with receiver, band and edge of the field of view in vector registers.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize -Icyclistsocialforce_amd/csrc -o packed_vs_plain_ubench tools/packed_vs_plain_ubench.hip
// Run once on the GPU box (a few milliseconds of work): ./packed_vs_plain_ubench > profiles/packed_vs_plain_ubench.txt
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#include "csf_field.h"

using csf::v2f;

#define ITER 1024
#define CHAIN_ITER 256

enum Row {
    FMA_V, MUL_V, ADD_V,              // independent streams, VGPR operands
    FMA_V_RSQ, MUL_V_RSQ, ADD_V_RSQ,  // ... with one v_rsq_f32 per eight instructions
    FMA_S, MUL_S, ADD_S,              // an SGPR pair (plain: an SGPR) as one operand
    FMA_S_RSQ,
    FMA_C, MUL_C,                     // inline constant (packed: op_sel_hi broadcasts it)
    FMA_C_RSQ,
    KEEP_IN, KEEP_FOV, FIELD,         // the dependent chains of csf_field.h, receiver in scalar registers
    KEEP_IN_V, KEEP_FOV_V, FIELD_V,   // ... receiver, band and edge of the field of view in vector registers
    N_ROWS
};

static const char *row_name[N_ROWS] = {
    "fma  vgpr pair", "mul  vgpr pair", "add  vgpr pair", "fma  vgpr pair + rsq/8", "mul  vgpr pair + rsq/8", "add  vgpr pair + rsq/8",
    "fma  sgpr pair", "mul  sgpr pair", "add  sgpr pair", "fma  sgpr pair + rsq/8", "fma  inline const", "mul  inline const",
    "fma  inline const + rsq/8", "chain keep_x2<inside>", "chain keep_x2<fov>", "chain field_twod_x2<full,near>",
    "chain keep<inside> recv vgpr", "chain keep<fov> recv vgpr", "chain field recv vgpr"};

// pairs of results of one wave (per lane): what the cycles are divided by
static double pairs_per_wave(int row) { return row >= KEEP_IN ? (double)CHAIN_ITER : (double)ITER * 8; }

template <int ROW, bool PACKED>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void bench(unsigned long long *dt, float *sink, float a, float b,
                                                                                        csf::PairConsts kc) {
    float acc = 0.f;
    unsigned long long t0, t1;
    if (ROW < KEEP_IN) {
        v2f p[8];
        const v2f pa = {a, a}, pb = {b, b};
        float sa = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(a)));
        v2f spa = {sa, sa};
#pragma unroll
        for (int i = 0; i < 8; i++) p[i] = v2f{a + i + threadIdx.x * 1e-3f, b + i};
        float xs[16];                  // the plain form's sixteen results
#pragma unroll
        for (int i = 0; i < 16; i++) xs[i] = i & 1 ? p[i >> 1].y : p[i >> 1].x;
        constexpr bool RSQ = ROW == FMA_V_RSQ || ROW == MUL_V_RSQ || ROW == ADD_V_RSQ || ROW == FMA_S_RSQ || ROW == FMA_C_RSQ;
        float rq = 1.5f + a;
        t0 = __builtin_amdgcn_s_memtime();
        for (int it = 0; it < ITER; it++) {
#pragma unroll
            for (int i = 0; i < 8; i++) {
                if (PACKED) {
                    if (ROW == FMA_V || ROW == FMA_V_RSQ) asm volatile("v_pk_fma_f32 %0, %0, %1, %2" : "+v"(p[i]) : "v"(pa), "v"(pb));
                    if (ROW == MUL_V || ROW == MUL_V_RSQ) asm volatile("v_pk_mul_f32 %0, %0, %1" : "+v"(p[i]) : "v"(pa));
                    if (ROW == ADD_V || ROW == ADD_V_RSQ) asm volatile("v_pk_add_f32 %0, %0, %1" : "+v"(p[i]) : "v"(pb));
                    if (ROW == FMA_S || ROW == FMA_S_RSQ) asm volatile("v_pk_fma_f32 %0, %0, %1, %2" : "+v"(p[i]) : "s"(spa), "v"(pb));
                    if (ROW == MUL_S) asm volatile("v_pk_mul_f32 %0, %0, %1" : "+v"(p[i]) : "s"(spa));
                    if (ROW == ADD_S) asm volatile("v_pk_add_f32 %0, %1, %0 neg_lo:[0,1] neg_hi:[0,1]" : "+v"(p[i]) : "s"(spa));
                    if (ROW == FMA_C || ROW == FMA_C_RSQ) asm volatile("v_pk_fma_f32 %0, %0, 0.5, 0.5 op_sel_hi:[1,0,0]" : "+v"(p[i]));
                    if (ROW == MUL_C) asm volatile("v_pk_mul_f32 %0, %0, 0.5 op_sel_hi:[1,0]" : "+v"(p[i]));
                    if (RSQ && i == 7) asm volatile("v_rsq_f32 %0, %0" : "+v"(rq));
                } else {
#pragma unroll
                    for (int h = 0; h < 2; h++) {
                        float &x = xs[2 * i + h];
                        if (ROW == FMA_V || ROW == FMA_V_RSQ) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(x) : "v"(a), "v"(b));
                        if (ROW == MUL_V || ROW == MUL_V_RSQ) asm volatile("v_mul_f32 %0, %0, %1" : "+v"(x) : "v"(a));
                        if (ROW == ADD_V || ROW == ADD_V_RSQ) asm volatile("v_add_f32 %0, %0, %1" : "+v"(x) : "v"(b));
                        if (ROW == FMA_S || ROW == FMA_S_RSQ) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(x) : "s"(sa), "v"(b));
                        if (ROW == MUL_S) asm volatile("v_mul_f32 %0, %1, %0" : "+v"(x) : "s"(sa));
                        if (ROW == ADD_S) asm volatile("v_sub_f32 %0, %1, %0" : "+v"(x) : "s"(sa));
                        if (ROW == FMA_C || ROW == FMA_C_RSQ) asm volatile("v_fma_f32 %0, %0, 0.5, 0.5" : "+v"(x));
                        if (ROW == MUL_C) asm volatile("v_mul_f32 %0, 0.5, %0" : "+v"(x));
                        if (RSQ && (i & 3) == 3 && h == 1) asm volatile("v_rsq_f32 %0, %0" : "+v"(rq));
                    }
                }
            }
        }
        t1 = __builtin_amdgcn_s_memtime();
#pragma unroll
        for (int i = 0; i < 8; i++) acc += PACKED ? p[i].x + p[i].y : xs[2 * i] + xs[2 * i + 1];
        acc += rq;
    } else {
        // the constants of the field in vector registers, as pair_cull_kernel holds them; the receiver in scalar or vector registers
        csf::PairConsts k = kc;
        asm volatile("" : "+v"(k.sg0), "+v"(k.sg1), "+v"(k.sg2), "+v"(k.sg3), "+v"(k.e0), "+v"(k.e1), "+v"(k.lf0), "+v"(k.kexp), "+v"(k.chs));
        asm volatile("" : "+v"(k.tA0), "+v"(k.tA1), "+v"(k.tB0), "+v"(k.tB1));
        constexpr bool RECV_V = ROW >= KEEP_IN_V;
        csf::Recv r{a, b, 0.8f * a, 0.6f * a};
        if (RECV_V) {
            asm volatile("" : "+v"(r.x), "+v"(r.y), "+v"(r.c), "+v"(r.s), "+v"(k.fovT0), "+v"(k.fovT1), "+v"(k.chk));
        } else {
            r.x = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(r.x)));
            r.y = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(r.y)));
            r.c = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(r.c)));
            r.s = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(r.s)));
        }
        const float l = (float)(threadIdx.x & 63);
        v2f qx = {3.f + 0.11f * l, 9.f - 0.07f * l}, qy = {2.f - 0.05f * l, 1.f + 0.13f * l};
        const v2f qc = {0.6f, -0.8f}, qs = {0.8f, 0.6f};
        float ax = 0.f, ay = 0.f;
        t0 = __builtin_amdgcn_s_memtime();
        for (int it = 0; it < CHAIN_ITER; it++) {
            if (ROW == FIELD || ROW == FIELD_V) {
                unsigned long long n0, n1;
                csf::field_twod_x2<true, true, !PACKED>(k, r, qx, qy, qc, qs, true, true, ax, ay, &n0, &n1);
                qx.x += 1e-3f * ax, qy.y += 1e-3f * ay;                     // the next pass waits for this one
                acc += (float)__builtin_popcountll(n0 | n1);
            } else {
                bool k0, k1, m0, m1;
                if (ROW == KEEP_IN || ROW == KEEP_IN_V) csf::keep_x2<false, false, !PACKED>(k, r, qx, qy, qc, qs, k0, k1, m0, m1);
                else csf::keep_x2<true, false, !PACKED>(k, r, qx, qy, qc, qs, k0, k1, m0, m1);
                qx.x += k0 ? 1e-3f : -1e-3f, qy.y += k1 ? 1e-3f : -1e-3f;
                acc += (m0 | m1) ? 1.f : 0.f;
            }
        }
        t1 = __builtin_amdgcn_s_memtime();
        acc += ax + ay + qx.x + qy.y;
    }
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    sink[gid] = acc;
    if ((threadIdx.x & 63) == 0) dt[gid >> 6] = t1 - t0;
}

static csf::PairConsts consts() {   // the TwoD field's defaults, roughly: only the instruction stream matters here
    csf::PairConsts k = {};
    k.sg0 = 0.3f, k.sg1 = 2.6f, k.sg2 = 0.2f, k.sg3 = 2.0f, k.e0 = 0.995f, k.e1 = 0.7f;
    k.lf0 = 2.8f, k.kexp = 1.4427f, k.chs = -0.25f, k.chk = 0.5f, k.fovT0 = 1e-6f, k.fovT1 = 1e-6f;
    k.tA0 = 3.f, k.tA1 = 20.f, k.tB0 = 2.f, k.tB1 = 15.f, k.rnear2 = 0.04f;
    return k;
}

template <int ROW, bool PACKED>
static double run(int waves_per_simd, int cus, unsigned long long *d_dt, float *d_sink) {
    const int blocks = cus * waves_per_simd;     // 4 waves per workgroup: one per SIMD
    const csf::PairConsts k = consts();
    for (int rep = 0; rep < 2; rep++) {          // (the first launch loads the code)
        hipLaunchKernelGGL((bench<ROW, PACKED>), dim3(blocks), dim3(256), 0, 0, d_dt, d_sink, 1.0001f, 0.5f, k);
        if (hipDeviceSynchronize() != hipSuccess) return -1.0;
    }
    std::vector<unsigned long long> dt((size_t)blocks * 4);
    if (hipMemcpy(dt.data(), d_dt, dt.size() * sizeof(dt[0]), hipMemcpyDeviceToHost) != hipSuccess) return -1.0;
    std::nth_element(dt.begin(), dt.begin() + dt.size() / 2, dt.end());
    return (double)dt[dt.size() / 2] / (pairs_per_wave(ROW) * waves_per_simd);
}

template <int ROW>
static bool row(int cus, unsigned long long *d_dt, float *d_sink) {
    printf("%-30s", row_name[ROW]);
    for (int w : {1, 2, 4, 8}) {
        const double pk = run<ROW, true>(w, cus, d_dt, d_sink), pl = run<ROW, false>(w, cus, d_dt, d_sink);
        if (pk < 0 || pl < 0) return false;
        printf(" | %7.2f %7.2f", pk, pl);
    }
    printf("\n");
    if constexpr (ROW + 1 < N_ROWS) return row<ROW + 1>(cus, d_dt, d_sink);
    return true;
}

int main() {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, 0) != hipSuccess) return 1;
    const int cus = prop.multiProcessorCount;
    unsigned long long *d_dt;
    float *d_sink;
    if (hipMalloc(&d_dt, (size_t)cus * 8 * 4 * sizeof(unsigned long long)) != hipSuccess) return 1;
    if (hipMalloc(&d_sink, (size_t)cus * 8 * 256 * sizeof(float)) != hipSuccess) return 1;
    printf("%s, %d CUs; SIMD cycles (s_memtime) per pair of f32 results, median over all waves; 4 x CUs x W waves of 64 lanes\n", prop.gcnArchName, cus);
    printf("chain rows: cycles per pass of two sources per lane, the pass's own transcendentals and the feedback of its result included\n");
    printf("%-30s | %15s | %15s | %15s | %15s\n", "waves per SIMD", "1", "2", "4", "8");
    printf("%-30s | %7s %7s | %7s %7s | %7s %7s | %7s %7s\n", "row", "packed", "2 plain", "packed", "2 plain", "packed", "2 plain", "packed", "2 plain");
    const bool ok = row<0>(cus, d_dt, d_sink);
    (void)hipFree(d_dt);
    (void)hipFree(d_sink);
    return ok ? 0 : 1;
}
