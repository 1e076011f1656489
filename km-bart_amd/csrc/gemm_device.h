// Device code shared by the GEMM translation units (gemm.hip, gemm_lean.hip, gemm_pair.hip and the role-split experiment,
// tools/experiments/gemm_rolesplit.hip): the LDS images' swizzle, the transposing fragment reads, LDS-DMA pieces and
// offsets, the L2 touch and the lean epilogue of the persistent kernels.  Kernels live in the .hip files.
#pragma once
#include <type_traits>
#include "common.h"
#include "diag.h"
#include "kernels.h"

// KMB_PLAIN_STORES (experiment builds, build.py --variant): default-policy stores in the persistent kernels' epilogues
// instead of non-temporal ones
#ifdef KMB_PLAIN_STORES
#define KMB_NT_STORE(v, p) (*(p) = (v))
#else
#define KMB_NT_STORE(v, p) __builtin_nontemporal_store(v, p)
#endif

// The L2 touch of the persistent kernels: a load whose result nobody reads.  Round 5: it is a 4-byte LDS-DMA into a dummy LDS word
// of the issuing wave (`lds`: 256 bytes that nothing reads while a touch can be in flight -- the wave's epilogue staging image,
// idle during the K loop) -- NO register destination.  Rounds 2-4 gave it a register: "=v" (a fresh value per touch: the allocator
// reused the register while the load was in flight -- wrong bits), one "+v" web (split under pressure: memory fault), then v255 with
// __attribute__((amdgpu_num_vgpr(255))), on the belief that the allocator then never hands out v255.  It does (found by grepping the ISA of every kernel with a touch for other uses of v255,
// round 5: the eight-wave and the two-workgroup kernels are compiled with all 256 registers, v255 among them -- the attribute does not
// cap a kernel whose budget waves_per_eu fixes); what kept the results right was the ORDER of the counted waits (a touch is older
// than the pieces the next wait leaves outstanding), not the register.  A touch still counts as one vector-memory operation, so the
// kernels' counted waits are unchanged; results are bit-identical (tests/test_gemm_variants_gpu.py).
// (inline asm, not __builtin_amdgcn_global_load_lds: the builtin spends eight scalar instructions per touch on turning the generic
//  LDS pointer into M0 -- measured -0.5...-1 % of a step; here M0 is saved, set from a 32-bit LDS address kept in a scalar
//  register and restored inside ONE statement, as the guide's glds16_asm recipe does.  `lds_u32`: kmb_lds_addr(ptr), wave-uniform.)
#define KMB_L2_TOUCH(voff, sbase, lds_u32)                                                                                    \
  do {                                                                                                                        \
    unsigned kmb_m0_keep_;                                                                                                    \
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2\n\ts_mov_b32 m0, %0"       \
                 : "=&s"(kmb_m0_keep_) : "v"(voff), "s"(sbase), "s"(lds_u32) : "memory");                                     \
  } while (0)
__device__ __forceinline__ unsigned kmb_lds_addr(const void* p) {   // the 32-bit LDS address of a (generic) pointer into shared memory, in a scalar register
  return (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(size_t)(__attribute__((address_space(3))) const void*)p);
}
namespace {

constexpr int BM = 128, BN = 128, BK = 64;

__device__ __forceinline__ int swz_nkc(int krow) { return (krow & 3) | (((krow >> 3) & 1) << 2); }

// fragment for MFMA 16x16x32: 16 rows (r = lane&15) x 32 k (8 per lane group g = lane>>4)
// The transposing LDS reads (`ds_read_b64_tr_b16`, the token-major operand of the data- and weight-gradient layouts) as INLINE ASM (late round 5).
// hipcc puts `s_waitcnt vmcnt(0)` in front of the first __builtin_amdgcn_ds_read_tr16_b64 behind an LDS-DMA issue: the intrinsic carries no memory
// operand, so the wait-count pass assumes it may read what the DMA is writing.  The K loops issue the NEXT stage's DMA pieces and then read fragments
// of the CURRENT one -- so in every kernel with a token-major operand the stage requested a moment ago was waited for at once: prefetch distance
// zero, two such stalls per K step in the weight-gradient kernel (found on the ISA: one counted wait per step in the K-contiguous kernels, two or
// three vmcnt(0) in the others; their matrix pipes were busy 29-40 % against 42 %).  As asm the compiler sees neither an LDS read (no wait in
// front) nor its result's latency (no wait before the use): the consumers' wait is an explicit `s_waitcnt lgkmcnt(0)` at the top of every
// sub-phase (KMB_TR_SYNC, fenced by sched_barriers: fragments are always consumed one sub-phase after they are requested) and behind the K loop of
// the persistent kernels (the next tile's first fragments live across the epilogue).  Sound only if no instruction names such a register between
// the read and the wait -- a property of the compiled code: tools/gemm_tr_asm_hazards.py walks the ISA's control-flow graph, and
// tests/test_cabi_cpu.py::test_gemm_asm_transposing_reads_are_waited_for runs it on every build.  Same arithmetic in the same order: outputs
// bit-identical to the intrinsic's (tools/gemm_tr_asm_ab.py: md5 per shape).  Kernels: v7 (+ the grouped weight gradients), v8, v11 with 256-wide
// tiles (four and eight waves) -- the ones compared on the GPU when this went in (round 5); v7d, the 128- / 192-wide v11 tiles and gemm_lean.hip:
// KMB_TR_ALL (round 6; gemm_lean.hip's L2 touch moved off v255 first -- with asm reads the allocator hands that register out).
// -DKMB_TR_BUILTIN: the intrinsic everywhere (A/B builds).  profiles/r05_gemm_transposing_reads_asm.md.
// Round 6: EVERY kernel (KMB_TR_ALL: also the four-stage kernel, the 128- / 192-wide persistent tiles and gemm_lean.hip) -- one GPU call compared
// the md5 of seven shapes x nine launch variants between the intrinsic build, round 5's partial build and this one: all identical and stable
// (profiles/r06_gemm_transposing_reads_all_variants.txt; the four-stage kernel's lone workgroups -33 %, the 128- / 192-wide weight gradients -12...-21 %).
#ifndef KMB_TR_BUILTIN
constexpr bool KMB_TR_ALL = true;
#else
constexpr bool KMB_TR_ALL = false;
#endif
#ifndef KMB_TR_BUILTIN
__device__ __forceinline__ s16x4 kmb_tr_read_asm(const char* ptr) {
  s16x4 t;
  const uint32_t a = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const char*)ptr;
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(t) : "v"(a));
  return t;
}
// the same read at `addr` (32-bit LDS address in a register) + a compile-time byte offset in the instruction's offset field: one address
// register serves every (kk, hh) of a fragment column (gemm_lean.hip: without it each of the 16 reads of a stage kept its own hoisted address)
template <int OFF>
__device__ __forceinline__ s16x4 kmb_tr_read_asm_off(uint32_t addr) {
  static_assert(OFF >= 0 && OFF < 65536, "ds offset field is 16 bits");
  s16x4 t;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(t) : "v"(addr), "n"(OFF));
  return t;
}
#define KMB_TR_SYNC()                                   \
  do {                                                  \
    __builtin_amdgcn_sched_barrier(0);                  \
    __builtin_amdgcn_s_waitcnt(0xC07F); /* lgkmcnt(0); the builtin, not asm: hipcc's own wait tracking then knows the LDS queue is empty (as asm it re-waited, lgkmcnt(0), in front of the next use of a plain fragment read -- right behind the asm reads just issued) */ \
    __builtin_amdgcn_sched_barrier(0);                  \
  } while (0)
#else
#define KMB_TR_SYNC() do { } while (0)
#endif

// A wave-uniform pointer forced into SGPRs: LDS-DMA pieces issued from it take the saddr + 32-bit-voffset form (no per-piece
// 64-bit VALU address arithmetic)
__device__ __forceinline__ const char* uniform_ptr(const char* ptr) {
  const uint64_t a = reinterpret_cast<uint64_t>(ptr);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
  return reinterpret_cast<const char*>(((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ void dma_piece(const char* gbase, uint32_t off, char* lds_dst) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gbase + off),
                                   (__attribute__((address_space(3))) void*)lds_dst, 16, 0, 0);
}

template <bool KC, int ROWS, bool ASM = false>
__device__ __forceinline__ bf16x8 read_frag3(const char* lds, int rowtile16, int kk, int r, int g) {
  if (KC) {
    const int row = rowtile16 * 16 + r;
    const int c = kk * 4 + g;
    return *reinterpret_cast<const bf16x8*>(lds + row * 128 + ((c ^ ((row >> 1) & 7)) << 4));
  } else {
    bf16x8 out;
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const int krow = kk * 32 + g * 8 + hh * 4 + (r >> 2);
      const int off = krow * (ROWS * 2) + ((rowtile16 ^ swz_nkc(krow)) << 5) + ((r & 3) << 3);
#ifndef KMB_TR_BUILTIN
      const s16x4 t = ASM ? kmb_tr_read_asm(lds + off) : __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(lds + off));
#else
      const s16x4 t = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (__attribute__((address_space(3))) s16x4*)(lds + off));
#endif
      out[hh * 4 + 0] = t[0]; out[hh * 4 + 1] = t[1]; out[hh * 4 + 2] = t[2]; out[hh * 4 + 3] = t[3];
    }
    return out;
  }
}

template <bool KC, int NP = 8>
__device__ __forceinline__ void dma_offsets256w4(uint32_t (&off)[NP], int ld, int r0, int R, int wave, int lane) {
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int piece = wave * NP + i;  // 4 * NP pieces of 1 KiB per tile (32 for 256 rows, 24 for a 192-row KC image)
    if (KC) {
      const int row = piece * 8 + (lane >> 3);
      const int c = (lane & 7) ^ ((row >> 1) & 7);
      int grow = r0 + row;
      grow = grow < R ? grow : R - 1;
      off[i] = (uint32_t)(((grow - r0) * ld + c * 8) * 2);
    } else {
      const int krow = piece * 2 + (lane >> 5);
      const int ps = lane & 31;
      const int c32 = (ps >> 1) ^ swz_nkc(krow);
      int m = r0 + c32 * 16 + (ps & 1) * 8;
      const int mlast = ((R - 1) >> 3) << 3;
      m = m < R ? m : mlast;
      off[i] = (uint32_t)((krow * ld + (m - r0)) * 2);
    }
  }
}

// The hot epilogue classes of v11, everything decided at compile time.  With ONE wave per SIMD nothing hides an
// instruction: the general body (run-time option tests, edge handling, spilled-SGPR reloads) costs ~450 instructions
// per 16-row chunk = 7 us per 256x256 tile (in-kernel stamps), as long as the tile's MFMAs at K = 256.  Interior wave
// blocks with a bf16 output only; same operation order as gemm_epilogue_body (bit-identical results).
//   BIAS: + bias[col];  SCALE: * col_scale (the whole wave block lies in the scaled columns);  ACT 1: GeLU (+ optional
//   pre-activation store), 2: * GeLU'(aux);  DROP: dropout mask (with ACT 1 also on the stored derivative);  RES: + residual;
//   CS: column sums.
template <bool BIAS, bool SCALE, int ACT, bool RES, bool DROP, bool CS, int WROWS, bool F32 = false, int NJ = 8>
__device__ __forceinline__ void v11_epilogue_lean(const KmbGemm& p, f32x4 (&acc)[8][NJ], float* ef, int lane, int r, int g,
                                                  int row0w, int col0w) {
  constexpr int WCOLS = NJ * 16;
  // lane map of the row-major pass: CL column-lanes of 8 columns x RPI rows per iteration, NIT iterations per 16-row chunk
  // (128- and 96-column blocks: 16 x 4, four iterations; the 8-wave kernel's 64-column blocks: 8 x 8, two iterations)
  constexpr int CL = WCOLS > 64 ? 16 : 8, RPI = 64 / CL, NIT = 16 / RPI, LDE = WCOLS > 64 ? 128 : 64;
  const int lr = lane / CL;
  // a 96-column wave block (256x192 tile) keeps the 128-column lane map: the last four column-lanes of every row group
  // redo column-lane 11's work on the same addresses (same values: harmless duplicate stores) instead of branching
  // a 96- / 48-column wave block keeps the 128- / 64-column lane map: the column-lanes past the block redo the last
  // column-lane's work on the same addresses (same values: harmless duplicate stores) instead of branching
  const int c8 = ((lane % CL) * 8 < WCOLS) ? (lane % CL) * 8 : WCOLS - 8;
  const int gcol = col0w + c8;
  kmb_f32x2 bias2[4], csum2[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    bias2[e] = BIAS ? kmb_f32x2{p.bias[gcol + 2 * e], p.bias[gcol + 2 * e + 1]} : kmb_f32x2{0.f, 0.f};
    csum2[e] = kmb_f32x2{0.f, 0.f};
  }
  const kmb_f32x2 scale2 = {p.col_scale, p.col_scale};
  const kmb_f32x2 dscale2 = {p.drop_scale, p.drop_scale};
  // staging write (transposed accumulators: lane (r, g) holds C[16 i + r][16 j + 4 g .. +3]) and read addresses
  // Swizzle of a staged row: its 16-byte groups XORed with the row's low three bits.  Writes: the 8 lanes of a ds_write_b128
  // group (8 rows, one column group) spread over all 32 banks.  Reads: a lane of the row-major pass reads its eight floats as
  // two ds_read_b128, and the 16 lanes of a read group (two rows of different parity) then cover all 64 banks.  (Rounds 1-3
  // XORed at 32-byte granularity: every read asked for the even 16-byte groups only and the writes for every other one --
  // two-way conflicts on both, 15-25 % of the LDS cycles of the forward kernels: tools/pmc_stalls.sh.)
  float* const wbase = ef + r * LDE;
  const int sw = (r & 7) << 2;
  auto stage = [&](const f32x4 (&a)[NJ]) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) *reinterpret_cast<f32x4*>(wbase + ((j * 16 + g * 4) ^ sw)) = a[j];
    asm volatile("" ::: "memory");
  };
  const float* rd[NIT];   // this lane's floats 0-3 of row-iteration it; floats 4-7 are rd_hi floats further (RPI is even: the row parity is lr's)
#pragma unroll
  for (int it = 0; it < NIT; ++it)
    rd[it] = ef + (lr + RPI * it) * LDE + (c8 ^ (((lr + RPI * it) & 7) << 2));
  const int rd_hi = (lr & 1) ? -4 : 4;
  // row pointers of this lane's first row; a row-iteration is 4 rows further, a chunk 16
  bf16_t* out = F32 ? nullptr : p.out_bf16 + (size_t)(row0w + lr) * p.ld_out_bf16 + gcol;
  float* out32 = F32 ? p.out_f32 + (size_t)(row0w + lr) * p.ld_out_f32 + gcol : nullptr;   // fp32 logits (ld % 4 == 0)
  bf16_t* pre = (ACT == 1 && p.preact != nullptr) ? p.preact + (size_t)(row0w + lr) * p.ld_preact + gcol : nullptr;
  const bf16_t* side = nullptr;   // residual (RES) or GeLU' argument (ACT 2): one 16-byte load per row
  size_t ld_side = 0;
  if (RES) { side = p.residual + (size_t)(row0w + lr) * p.ld_res + gcol; ld_side = (size_t)p.ld_res; }
  if (ACT == 2) { side = p.aux + (size_t)(row0w + lr) * p.ld_aux + gcol; ld_side = (size_t)p.ld_aux; }
  constexpr bool SIDE = RES || ACT == 2;
  static_assert(!(RES && ACT == 2), "one side stream");
  // Side loads run two chunks ahead of their use (a chunk is ~0.3 us, an HBM miss longer).  The chunks are walked in pairs:
  // even chunks keep their side values in sE / hE, odd ones in sO / hO; a chunk first consumes its registers (unpacks them)
  // and then requests chunk i + 2 into the SAME registers, so the loop-carried value is defined by the load itself.  (Rounds
  // 1-3 rotated three register sets, s0 <- s1 <- s2, at the bottom of a one-chunk loop: the copy s1 <- s2 is a USE of the load
  // issued in that same iteration, so hipcc put `s_waitcnt vmcnt(0)` into every chunk -- the prefetch distance was zero and
  // each chunk also waited for its own stores: 10 us of the fc2 data-gradient tile's epilogue, tools/epilogue_burst.py.)
  // The eight-wave kernels (NIT = 2: 128 registers in all; with the pair loop they spilled, and a scratch access in the K
  // loop breaks its counted vmcnt waits) use ONE register set and a one-chunk distance: consume, request chunk i + 1, compute
  // chunk i -- their second wave per SIMD covers the rest.
  constexpr bool PAIRS = NIT == 4;
  constexpr int AHEAD = PAIRS ? 2 : 1;
  u32x4 sE[NIT];
  [[maybe_unused]] u32x4 sO[NIT];
  if (SIDE) {
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      sE[it] = *reinterpret_cast<const u32x4*>(side + (size_t)(RPI * it) * ld_side);
      if constexpr (PAIRS) sO[it] = *reinterpret_cast<const u32x4*>(side + (size_t)(16 + RPI * it) * ld_side);
    }
  }
  // act 5: the rows' shifts, loaded like the side operand two chunks ahead of their use (a load at the point of use exposed
  // its latency in every row-iteration: the head's forward GEMM 2.24 -> 3.19 ms)
  float hE[NIT];
  [[maybe_unused]] float hO[NIT];
  const float* shift_base = ACT == 5 ? p.row_shift + row0w + lr : nullptr;
  if constexpr (ACT == 5) {
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      hE[it] = shift_base[RPI * it];
      if constexpr (PAIRS) hO[it] = shift_base[16 + RPI * it];
    }
  }
  auto stage_chunk = [&](int i) {
    switch (i) {   // static accumulator indices in every arm (a run-time index would put acc in scratch)
      case 0: stage(acc[0]); break;
      case 1: stage(acc[1]); break;
      case 2: stage(acc[2]); break;
      case 3: stage(acc[3]); break;
      case 4: stage(acc[4]); break;
      case 5: stage(acc[5]); break;
      case 6: stage(acc[6]); break;
      default: stage(acc[7]); break;
    }
  };
  static_assert((WROWS / 16) % 2 == 0, "chunks are walked in pairs");
  auto chunk = [&](const int i, u32x4 (&sv)[NIT], float (&hv)[NIT]) {
    // this chunk's side values out of their registers, then chunk i + 2's requested into them (the last two chunks re-read
    // rows that are in cache; never used)
    [[maybe_unused]] float su[SIDE ? NIT : 1][8];
    [[maybe_unused]] float hc[ACT == 5 ? NIT : 1];
    const int ahead = i + AHEAD < WROWS / 16 ? i + AHEAD : WROWS / 16 - 1;
    if (SIDE) {
#pragma unroll
      for (int it = 0; it < NIT; ++it) unpack8(sv[it], su[it]);
      __builtin_amdgcn_sched_barrier(0);   // the unpacks stay in front of the reload of their source registers
#pragma unroll
      for (int it = 0; it < NIT; ++it) sv[it] = *reinterpret_cast<const u32x4*>(side + (size_t)(16 * ahead + RPI * it) * ld_side);
    }
    if constexpr (ACT == 5) {
#pragma unroll
      for (int it = 0; it < NIT; ++it) hc[it] = hv[it];
#pragma unroll
      for (int it = 0; it < NIT; ++it) asm volatile("" : "+v"(hc[it]));   // a value of its own, not an alias of the register being reloaded
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int it = 0; it < NIT; ++it) hv[it] = shift_base[16 * ahead + RPI * it];
    }
    // this chunk's rows out of LDS first, then the next chunk's accumulators into the same image: the LDS executes
    // a wave's accesses in order, so the writes queue behind the reads and their latency hides under this chunk's math
    f32x4 lo4[NIT], hi4[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      lo4[it] = *reinterpret_cast<const f32x4*>(rd[it]);
      hi4[it] = *reinterpret_cast<const f32x4*>(rd[it] + rd_hi);
    }
    asm volatile("" ::: "memory");
    if (i + 1 < WROWS / 16) stage_chunk(i + 1);
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const f32x4 lo = lo4[it];
      const f32x4 hi = hi4[it];
      kmb_f32x2 v[4] = {{lo[0], lo[1]}, {lo[2], lo[3]}, {hi[0], hi[1]}, {hi[2], hi[3]}};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (BIAS) v[e] = v[e] + bias2[e];
        if (SCALE) v[e] = v[e] * scale2;
      }
      const size_t roff = (size_t)(16 * i + RPI * it);
      if constexpr (ACT == 5) {
        // tied-head cross-entropy: exp(v - shift[row]) is what is stored; the row's fp32 sum over this wave block and the
        // shifted value at the label's column go to the side buffers (see KmbGemm)
        static_assert(ACT != 5 || WCOLS == 64 || WCOLS == 128, "act 5: 64- or 128-column wave blocks");
        const int grow = row0w + lr + 16 * i + RPI * it;
        const float c = hc[it];
        const kmb_f32x2 c2 = {c, c};
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] - c2;
        if (p.pick_col != nullptr) {   // uniform; optional (the engine does without: the shift IS the label's logit)
          const int rel = (int)((long long)p.pick_col[grow] - (long long)gcol);   // the label's column relative to this lane's eight
          if (rel >= 0 && rel < 8) {
            float picked = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              if (rel == 2 * e) picked = v[e][0];
              if (rel == 2 * e + 1) picked = v[e][1];
            }
            p.pick_out[grow] = picked;
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          // 2^115 bounds a stored value and a 50k-column row sum inside fp32 / bf16: a logit more than 80 above the label's (a
          // row whose loss exceeds 80 nats) saturates instead of turning the row's sum, loss and gradients into inf / NaN
          const kmb_f32x2 t = v[e] * 1.4426950408889634f;
          v[e] = kmb_f32x2{__builtin_amdgcn_exp2f(fminf(t[0], 115.f)), __builtin_amdgcn_exp2f(fminf(t[1], 115.f))};
        }
        float sum = (v[0][0] + v[0][1]) + (v[1][0] + v[1][1]) + ((v[2][0] + v[2][1]) + (v[3][0] + v[3][1]));
#pragma unroll
        for (int o = 1; o < CL; o <<= 1) sum += __shfl_xor(sum, o);   // the CL column-lanes of a row are consecutive lanes
        if ((lane % CL) == 0) {
          float* slot = p.row_sums + (size_t)grow * p.row_sums_ld + (col0w >> 6);
          slot[0] = sum;
          if (WCOLS == 128) slot[1] = 0.f;
        }
      } else if (ACT == 1) {
        // DROP (activation dropout): m = keep ? drop_scale : 0 goes into the output AND the stored derivative, so that what
        // backward multiplies by (ACT 2) is d/da of m * GeLU(a).  One hash per column pair decides both.  The hashes are taken
        // behind the GeLU arithmetic, when the derivative is already packed to bf16 (its eight registers are four by then: the
        // epilogue's register peak stays the GeLU evaluation's), and a dropped derivative is cleared in its packed word.
        // (gcol is a multiple of 8: a pair's column term is drop_colterm(gcol) + e * the term's multiplier.)
        [[maybe_unused]] uint32_t hsh[4];
        [[maybe_unused]] auto draw = [&]() {
          uint32_t rw = (uint32_t)(row0w + lr + 16 * i + RPI * it), cw = (uint32_t)gcol;
          asm volatile("" : "+v"(rw), "+v"(cw));   // nothing of the hashes is hoisted out of the tile loop into registers that live across the K loop
          const uint32_t rowterm = rw * 0x9E3779B1u;
          const uint32_t ct0 = drop_colterm(cw);
#pragma unroll
          for (int e = 0; e < 4; ++e) hsh[e] = kmb_hash32(rowterm ^ (ct0 + (uint32_t)e * 0x85EBCA77u) ^ p.drop_seed);
        };
        if (pre != nullptr) {   // GeLU and GeLU' from one evaluation; the derivative is stored for backward (ACT 2)
          kmb_f32x2 dv[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            kmb_f32x2 y;
            gelu_both2(v[e], y, dv[e]);
            v[e] = y;
            if constexpr (DROP) dv[e] = dv[e] * dscale2;
          }
          u32x4 pk = {pack2bf(dv[0][0], dv[0][1]), pack2bf(dv[1][0], dv[1][1]), pack2bf(dv[2][0], dv[2][1]), pack2bf(dv[3][0], dv[3][1])};
          if constexpr (DROP) {
            draw();
#pragma unroll
            for (int e = 0; e < 4; ++e)
              pk[e] = ((hsh[e] & 0xffffu) >= p.drop_thr16 ? pk[e] & 0xffffu : 0u) | ((hsh[e] >> 16) >= p.drop_thr16 ? pk[e] & 0xffff0000u : 0u);
          }
          KMB_NT_STORE(pk, reinterpret_cast<u32x4*>(pre + roff * p.ld_preact));
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = gelu2(v[e]);
          if constexpr (DROP) draw();
        }
        if constexpr (DROP) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const kmb_f32x2 kept = v[e] * dscale2;
            v[e] = kmb_f32x2{(hsh[e] & 0xffffu) >= p.drop_thr16 ? kept[0] : 0.f, (hsh[e] >> 16) >= p.drop_thr16 ? kept[1] : 0.f};
          }
        }
      } else if (ACT == 2) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] * kmb_f32x2{su[it][2 * e], su[it][2 * e + 1]};
      }
      if (DROP && ACT != 1) {   // (ACT 1 has drawn above: never a second time)
        const uint32_t grow = (uint32_t)(row0w + lr + 16 * i + RPI * it);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const kmb_f32x2 kept = v[e] * dscale2;
          v[e][0] = drop_keep(p.drop_seed, grow, (uint32_t)(gcol + 2 * e), p.drop_thr16) ? kept[0] : 0.f;
          v[e][1] = drop_keep(p.drop_seed, grow, (uint32_t)(gcol + 2 * e + 1), p.drop_thr16) ? kept[1] : 0.f;
        }
      }
      if (RES) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] + kmb_f32x2{su[it][2 * e], su[it][2 * e + 1]};
      }
      if (CS) {
#pragma unroll
        for (int e = 0; e < 4; ++e) csum2[e] = csum2[e] + v[e];
      }
      if (F32) {
        float* o = out32 + roff * p.ld_out_f32;
        KMB_NT_STORE((f32x4{v[0][0], v[0][1], v[1][0], v[1][1]}), reinterpret_cast<f32x4*>(o));
        KMB_NT_STORE((f32x4{v[2][0], v[2][1], v[3][0], v[3][1]}), reinterpret_cast<f32x4*>(o + 4));
      } else {
        const u32x4 pk = {pack2bf(v[0][0], v[0][1]), pack2bf(v[1][0], v[1][1]), pack2bf(v[2][0], v[2][1]), pack2bf(v[3][0], v[3][1])};
#ifdef KMB_PLAIN_FFN_OUT   // experiment build: the FFN's wide activations (GeLU output, its gradient) with default-policy stores
        if (ACT == 1 || ACT == 2) *reinterpret_cast<u32x4*>(out + roff * p.ld_out_bf16) = pk;
        else KMB_NT_STORE(pk, reinterpret_cast<u32x4*>(out + roff * p.ld_out_bf16));
#else
        KMB_NT_STORE(pk, reinterpret_cast<u32x4*>(out + roff * p.ld_out_bf16));
#endif
      }
    }
  };
  stage_chunk(0);
  if constexpr (PAIRS) {
#pragma unroll 1
    for (int i = 0; i < WROWS / 16; i += 2) {
      chunk(i, sE, hE);
      chunk(i + 1, sO, hO);
    }
  } else {
#pragma unroll 1
    for (int i = 0; i < WROWS / 16; ++i) chunk(i, sE, hE);
  }
  if (CS) {
    float csum[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) { csum[2 * e] = csum2[e][0]; csum[2 * e + 1] = csum2[e][1]; }
#pragma unroll
    for (int e = 0; e < 8; ++e) {   // fold the row-lanes
      if (CL == 8) csum[e] += __shfl_xor(csum[e], 8);
      csum[e] += __shfl_xor(csum[e], 16);
      csum[e] += __shfl_xor(csum[e], 32);
    }
    if (lane < CL) {
      const int prow = row0w >> 6;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        p.colsum[(size_t)prow * p.N + gcol + e] = csum[e];
        if (WROWS == 128) p.colsum[(size_t)(prow + 1) * p.N + gcol + e] = 0.f;
      }
    }
  }
}

}  // namespace
