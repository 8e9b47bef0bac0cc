// Build-mode switch for the kernel sources.
//   default      : real HIP for gfx950 (hipcc --offload-arch=gfx950) — the product.
//   -DPLONK_EMU  : tests/emu/hip_emu.h, a fiber-based single-source emulation of the HIP execution
//                  model on the host, used ONLY by the CPU test-suite (tests/emu/) to check kernel
//                  index/barrier logic in a container without a GPU.  Never built into
//                  libplonk_hip.so and never loaded by the plonkathon_amd package.
#pragma once
#ifdef PLONK_EMU
#include "hip_emu.h"
#else
#include <hip/hip_runtime.h>
#define PLONK_HD __host__ __device__ __forceinline__
// The 254-bit multiply is ~330 instructions; inlining every call makes the hot kernels 60-300 KB of
// code against a 64 KB instruction cache.  PLONK_FP_CALL = out-of-line (one copy per kernel image).
// out-of-line helper for large, rarely-hot bodies (Keccak-f: inlining it at every sponge call site made
// transcript_kernel 694 KB)
#define PLONK_HD_NOINLINE __host__ __device__ inline __attribute__((noinline))
#ifdef PLONK_FP_OUTLINE
#define PLONK_FP_CALL __host__ __device__ __attribute__((noinline))
#else
#define PLONK_FP_CALL __host__ __device__ __forceinline__
#endif
#define PLONK_DEV __device__ __forceinline__
// a lambda whose body must be inlined at every call (large bodies otherwise become calls, and the arrays they touch move to scratch)
#define PLONK_LAMBDA_INLINE __attribute__((always_inline))
#define PLONK_KERNEL(...) HIP_KERNEL_NAME(__VA_ARGS__)
#define PLONK_LAUNCH(kern, grid, block, shmem, stream, ...) \
    hipLaunchKernelGGL(kern, grid, block, shmem, stream, __VA_ARGS__)
// stops the scheduler from interleaving independent big-integer ops (which multiplies live registers)
#ifdef __HIP_DEVICE_COMPILE__
#define PLONK_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#else
#define PLONK_SCHED_FENCE() ((void)0)
#endif
#define PLONK_DYN_SMEM(name) extern __shared__ __attribute__((aligned(16))) unsigned char name[]
#endif

// PLONK_SHORT_KERNEL(): the first statement of every SHORT kernel on a batch's serial path — wave priority 3 for the wave's life.
// The rule.  A batch is one stream, and a stream is one serial lane: while it sits in a kernel that does almost no work it feeds the
// chip nothing.  Beside another stream's accumulation (msm_comb_rows_kernel: waves that live ~0.6 ms and keep 93 % of a SIMD's VALU
// issue slots busy) such a kernel's waves are always the youngest on their SIMD, and issue is arbitrated by priority, then age: they
// get the leftover slots and run three to five times their lone duration.  Priority outranks age, so these kernels take it:
//   transcript_kernel; the comb MSM's digits, row-sum, column-sum, finalize and recovery kernels; every scan kernel of prover_scans.h;
//   linearisation_weights / linearisation / gate_check / quotient_combine / pi_coeffs / pi_coset / pack_proofs / pack_status;
//   the blinding correction kernels.
// Together they issue under 5 % of a step's instructions, which is all the accumulation can lose to them.  The accumulation kernels
// stay at priority 0: msm_comb_rows_kernel, msm_comb_kernel, the bucket and window accumulation kernels.
// PLONK_WORK_KERNEL(): priority 1 for the other kernels that ARE a step's work but sit on a batch's serial path all the same — the
// transforms (ntt_wavel_kernel, ntt_wavel_column_kernel, ntt_pass_radix2_kernel) and quotient_kernel, 14 % of the step's instructions.
// Measured, not argued: with them at 0 the step was 201.95 ms, at 1 it was 199.97 (profiles/short_kernel_priority.json, variants).
// The instruction is scalar and ignores EXEC: both macros are placed unconditionally, never under a branch.
// Nothing in the host and emulator builds.  (A/B builds: make EXTRA="-DPLONK_SHORT_KERNEL_PRIORITY=0 -DPLONK_WORK_KERNEL_PRIORITY=0".)
#ifndef PLONK_SHORT_KERNEL_PRIORITY
#define PLONK_SHORT_KERNEL_PRIORITY 3
#endif
#ifndef PLONK_WORK_KERNEL_PRIORITY
#define PLONK_WORK_KERNEL_PRIORITY 1
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define PLONK_SHORT_KERNEL() __builtin_amdgcn_s_setprio(PLONK_SHORT_KERNEL_PRIORITY)
#define PLONK_WORK_KERNEL() __builtin_amdgcn_s_setprio(PLONK_WORK_KERNEL_PRIORITY)
#else
#define PLONK_SHORT_KERNEL() ((void)0)
#define PLONK_WORK_KERNEL() ((void)0)
#endif

// PLONK_BESIDE_ACC(lanes, bit): the launch bounds of a short kernel that has a SMALL FORM — compiled for five waves per SIMD, at most
// 96 VGPRs, what is free on a SIMD beside four waves of msm_comb_rows_kernel (104 each of 512), so that its workgroups need not wait
// for a whole accumulation workgroup to retire.  A kernel takes the small form where bit `bit` of PLONK_SMALL_FORMS is set: 1
// msm_comb_finalize_kernel, 2 msm_comb_rowsum_kernel, 4 grand_product_kernel, 8 eval_kernel and eval_seg_kernel, 16
// linearisation_weights_kernel, 32 msm_comb_slow_kernel, 64 quotient_kernel.  The bit switches launch bounds only.  eval_kernel's
// small form exists since the evaluations walk their rows in passes and add up inside the waves (prover_scans.h: 92 VGPRs, no
// scratch, 896 bytes of LDS, where seven chains at once and a tree over 56 KB of LDS held a SIMD to two waves whatever was asked);
// msm_comb_slow_kernel's since its rare branch is inline (the out-of-line helper alone held 97 registers).  Each was decided by
// measurement — a form is kept if its in-step mean falls by more than its lone mean grows (profiles/short_kernel_priority.txt,
// profiles/serial_path_small_forms.txt: registers, scratch and durations of both forms); the default is the set that was kept: all
// seven.  (A/B builds: make EXTRA=-DPLONK_SMALL_FORMS=0.)
#ifndef PLONK_SMALL_FORMS
#define PLONK_SMALL_FORMS 127
#endif
#define PLONK_BESIDE_ACC(lanes, bit) PLONK_BESIDE_ACC_##bit(lanes)
#if (PLONK_SMALL_FORMS) & 1
#define PLONK_BESIDE_ACC_1(lanes) __launch_bounds__(lanes, 5)
#else
#define PLONK_BESIDE_ACC_1(lanes) __launch_bounds__(lanes)
#endif
#if (PLONK_SMALL_FORMS) & 2
#define PLONK_BESIDE_ACC_2(lanes) __launch_bounds__(lanes, 5)
#else
#define PLONK_BESIDE_ACC_2(lanes) __launch_bounds__(lanes)
#endif
#if (PLONK_SMALL_FORMS) & 4
#define PLONK_BESIDE_ACC_4(lanes) __launch_bounds__(lanes, 5)
#else
#define PLONK_BESIDE_ACC_4(lanes) __launch_bounds__(lanes)
#endif
#if (PLONK_SMALL_FORMS) & 16
#define PLONK_BESIDE_ACC_16(lanes) __launch_bounds__(lanes, 5)
#else
#define PLONK_BESIDE_ACC_16(lanes) __launch_bounds__(lanes)
#endif
#if (PLONK_SMALL_FORMS) & 8
#define PLONK_BESIDE_ACC_8(lanes) __launch_bounds__(lanes, 5)
#else
#define PLONK_BESIDE_ACC_8(lanes) __launch_bounds__(lanes)
#endif
#if (PLONK_SMALL_FORMS) & 32
#define PLONK_BESIDE_ACC_32(lanes) __launch_bounds__(lanes, 5)
#else
#define PLONK_BESIDE_ACC_32(lanes) __launch_bounds__(lanes)
#endif
#if (PLONK_SMALL_FORMS) & 64
#define PLONK_BESIDE_ACC_64(lanes) __launch_bounds__(lanes, 5)
#else
#define PLONK_BESIDE_ACC_64(lanes) __launch_bounds__(lanes)
#endif

// PLONK_CHAIN(acc): an empty statement that merely USES the running 64-bit column sum of a product-scanning
// multiplication.  The second use makes every partial sum a leaf for LLVM's reassociation, which otherwise sums a
// column's products from zero and adds the carry of the previous column last — one v_lshl_add_u64 per column, 16 per
// multiplication (5-7 % of the instructions of every ALU-bound kernel here).  With the chain kept as written the carry is
// the addend of the column's first v_mad_u64_u32.  Emits no instruction.  The statements of one multiplication are
// threaded through a scalar token (BEGIN ... END ties it to a result word) instead of being `volatile`, so that the
// scheduler may still interleave independent multiplications: volatile statements keep program order, which cost the
// 3-waves-per-SIMD NTT kernel 4 % at saturation, and were no faster for the MSM loop (profiles/r02_p_chain_ab.txt, r02_q).
#if defined(__HIP_DEVICE_COMPILE__)
#define PLONK_CHAIN_BEGIN() uint32_t plonk_chain_tok = 0
#define PLONK_CHAIN(acc) asm("" : "=s"(plonk_chain_tok) : "v"(acc), "0"(plonk_chain_tok))
#define PLONK_CHAIN_END(word) asm("" : "+v"(word) : "s"(plonk_chain_tok))
#else
#define PLONK_CHAIN_BEGIN() ((void)0)
#define PLONK_CHAIN(acc) ((void)0)
#define PLONK_CHAIN_END(word) ((void)0)
#endif
