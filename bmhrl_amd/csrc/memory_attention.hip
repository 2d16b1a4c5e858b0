// Few-query attention over a long memory, core of the fusion layers' caption -> audio / video attentions in the absorbed
// form (model/bm_hrl_agent.py:87-101 through functional.PairMemAttnFn: Q' = Q Wk per head, keys = values = the memory rows):
// L <= 32 caption positions of a (sample, head) against Sk <= 896 memory rows of width dm (128 audio / 1024 video).
//
// On the batched-GEMM path the core is score GEMM + row softmax + context GEMM forward and dP GEMM + row kernel + dQ' GEMM
// backward, six launches per block whose 30-row outputs waste most of every tile.  Here a workgroup owns one (sample, head)
// and runs ONE template in two modes:
//
//   pass 1   T^T[key][q] = mem[key] . X[q]      X = Q' (forward) or dCx (backward), staged in LDS; the wave's key tiles
//            (tile t to wave t mod 8) stay in registers, the key rows fed in the order that makes the accumulator layout the
//            B-operand layout of pass 2 (as in small_attention.hip); the memory rows come through the wave's LDS ring
//   middle   forward : scale, -1e9 at masked keys, softmax over ALL keys (register partials -> one LDS exchange between the
//                      eight waves), P -> bf16 -> HBM (the backward and d(mem) need it) and an LDS image
//            backward: dS = scale P (dP - sum_k P dP) with P read back in the same layout, 0 at masked keys, -> HBM and LDS
//   pass 2   Y^T[d][q] = memT[d] . E[q]         E = P / dS rows from the LDS image, memT = the memory transposed once per step
//            (functional.StepScratch.memo_mem) so that the reduction over keys is contiguous for the MFMA A operand; the d
//            tiles are dealt to the waves and streamed like the rows of pass 1, the output rows leave through an LDS image as
//            whole 16-byte pieces
//
// Each (sample, head) streams the memory once per pass (2 x 512 KB for the video side), out of L2.  Both streams go through
// LDS (MaStream below): direct-to-LDS loads of 8 rows x 128 bytes -- whole cache lines -- into a ring private to the wave, the
// A fragments by ds_read_b128 from the XOR-swizzled image, counted vmcnt waits, no barrier inside a stream.  The k order of every
// product, the key <-> MFMA-slot map and the accumulator -> B-operand trick are those of the register-streaming loops this
// replaced (r03 - r05: the A fragments loaded from global memory in MFMA layout, 32 rows x 32 bytes per wave instruction),
// so the outputs are theirs bit for bit (bench.py --dump-outputs under BMHRL_DETERMINISTIC=1: loss and parameters identical).
//
// MEASURED alone (tests/bench_memattn.py, forward / backward, one process): register streaming r03 video side 44 / 46 us
// against 35 us for the three launches it replaces, audio side 28 / 31 against 33; r04 with the XCD-aware block map below (all
// heads and both stacks of a sample on one XCD: the memory leaves the Infinity Cache once instead of four times) 38.8 / 44.2 and
// 23.0 / 24.6 us, the GEMM path 29.9 / 33.2 us; deeper unrolling of those load streams (32 loads in flight per wave) changed
// nothing.  r06, same box and run order: register streaming 42.5 / 41.8 and 23.3 / 24.8 us, the LDS rings 23.5 / 25.1 and
// 20.3 / 21.4 us, the GEMM path 30.6 / 32.0 us -- faster than the three launches in both directions at both shapes.  L2 read
// requests per launch (TCC_READ_sum, mean over both shapes) 1.16 M -> 0.81 M against 0.76 M lines that the operands hold: the
// fragment-shaped loads re-fetched about every second line from L2 (not every line four times), the rest of the gain is the
// access shape in front of the L1.  What bounds it now is not load latency: a ring of 2 units gives the video side what 4 give
// (23.7 / 25.6 us), a ring of 1 unit 28.2 / 28.3, and the audio side is the same at every depth; a workgroup moves 3 MB through
// its LDS on the video side (the fill, the A and the B fragment reads), about 10 us of the LDS port, next to the launch, the X
// staging, the middle and the output image, which were not separated.  In the step (bench.py, parent and change alternating)
// 4.783 / 4.803 -> 4.697 / 4.689 ms; the eight calls 0.344 -> 0.215 ms of kernel time.
// Default since r04 (functional.FUSED_MEMATTN; BMHRL_FUSED_MEMATTN=0 selects the GEMM path; parity:
// tests/test_memory_attention_gpu.py, tests/test_memory_attention_stream_gpu.py, tests/test_blocks_gpu.py).
#include "../../include/bmhrl_hip.h"
#include "common.h"

namespace {

// eight waves, two per SIMD: while one waits for its ring the other multiplies
constexpr int MA_WAVES = 8, MA_THREADS = 64 * MA_WAVES;
constexpr int MA_MAXD = 1024, MA_MAXK = 896, MA_PAD = 8, MA_NT = (MA_MAXK / 32 + MA_WAVES - 1) / MA_WAVES;   // <= 4 tiles per wave and pass
static_assert(MA_MAXD / 32 <= MA_NT * MA_WAVES, "pass 2 keeps a wave's d-tiles in the same accumulators");

// ---- LDS map (one array: a second __shared__ object next to direct-to-LDS loads makes the compiler drain them)
//   [0, xs)              Xs   X rows [32][dm + 8]; after pass 2 the output image
//   [es, es + es_bytes)  Es   P / dS rows [32][Skp + 8], written after pass 1
//   [MA_LDS - MA_RED, .) red  the softmax / delta exchange
// The ring of pass 1 is everything above Xs but red (Es does not exist yet), the ring of pass 2 everything below Es (Xs is
// dead after pass 1; the output tiles wait in registers for a barrier).  A wave owns 1/8 of a ring, cut into units.
constexpr int MA_LDS = 160 * 1024, MA_RED = MA_WAVES * 32 * 2 * 4;
constexpr int MA_UNIT = 4096, MA_MAXU = 4;      // a unit: 32 rows x 128 bytes = four 1 KiB pieces; units in flight per wave
__host__ __device__ constexpr int ma_xs_bytes(int dm) { return 32 * (dm + MA_PAD) * 2; }
__host__ __device__ constexpr int ma_es_off(int Skp) { return MA_LDS - MA_RED - 32 * (Skp + MA_PAD) * 2; }
__host__ __device__ constexpr int ma_units(int ring_bytes) {
  return ring_bytes / (MA_WAVES * MA_UNIT) < MA_MAXU ? ring_bytes / (MA_WAVES * MA_UNIT) : MA_MAXU;
}
__host__ __device__ constexpr int ma_units1(int dm) { return ma_units(MA_LDS - MA_RED - ma_xs_bytes(dm)); }
__host__ __device__ constexpr int ma_units2(int Skp) { return ma_units(ma_es_off(Skp)); }
// both shrink as dm / Sk grow, so the maxima bmhrl_memory_attention_ok admits are the shortest rings there are (2 and 3 units)
static_assert(ma_units1(MA_MAXD) >= 1 && ma_units2(MA_MAXK) >= 1, "every admitted shape has a ring");
static_assert(ma_xs_bytes(MA_MAXD) <= ma_es_off(MA_MAXK), "Xs and Es do not meet");

struct MemAttnArgs {
  const bf16_t* X; long ldx;            // row (b2 * L + q) * ldx + h * dm
  const bf16_t* mem; long mem_sb;       // + (b2 % nb) * mem_sb + key * dm
  const bf16_t* memT; long memT_sb; int ldt;   // + (b2 % nb) * memT_sb + d * ldt + key   (columns >= Sk zero up to a multiple of 16)
  bf16_t* PD; long pd_row; long pd_slot;       // + (b2 * L + q) * pd_row + slot * pd_slot + h * Skp + key
  bf16_t* Y; long ldy;                  // row (b2 * L + q) * ldy + h * dm
  const uint8_t* mask; long mask_sb;    // + b2 * mask_sb + key
  int nb, H, L, Sk, Skp, dm;
  float scale;
  int xcd_map;                          // 1: block -> (sample, head) through the XCD-aware map (B2 a multiple of 8)
};

__device__ __forceinline__ int ma_key_of_row(int rho) {
  return 8 * ((rho >> 2) & 1) + (rho & 3) + 4 * ((rho >> 3) & 1) + 16 * ((rho >> 4) & 1);
}

template <int IMM>
__device__ __forceinline__ bf16x8 ma_lds128(unsigned addr) {     // (asm: the compiler would drain the ring before a read it sees)
  bf16x8 r;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(IMM));
  return r;
}
// at most `units` of this wave's units (four pieces each) may still be in flight; a wave's loads land in order
__device__ __forceinline__ void ma_wait_units(int units) {
  if (units >= 3) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
  else if (units == 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  else if (units == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// One pass over a row-major matrix as the MFMA A operand: acc[i] += M[tile wave + 8 i] . B over the columns, in column order.
// A unit is 32 rows x 64 columns, filled by four direct-to-LDS loads of 8 rows x 128 bytes (whole lines); its image has
// 128-byte rows, the 16-byte chunk c of row r at slot c ^ ((r >> 1) & 7): the swizzle is on the SOURCE address (the loads
// write lane-linearly) and on the read, which makes the ds_read_b128 of a k-step conflict-free.  The ring is private to
// the wave, so its own counted vmcnt orders a read behind the fill and its own lgkmcnt(0) a refill behind the last read:
// no barrier inside the stream (a cooperative ring would add one per unit and save nothing: no tile is shared).
// KEYMAP (pass 1): image row rho holds key ma_key_of_row(rho) of the tile, rows past the memory are clamped.
template <bool KEYMAP>
struct MaStream {
  const char* base; unsigned row_bytes; int ncol, row_max;   // the matrix; loads are clamped to its rows and columns
  int ntw, upt, ks_last, U;          // this wave's tiles, units per tile, k-steps of a tile's last unit, units of the ring
  char* ring; unsigned a_addr[4], b_addr;                    // the ring; LDS byte addresses of the lane's fragments
  int wave, lane;
  int ni, nu, ns, nleft;             // the next unit to issue: tile, unit, slot; units not issued yet

  __device__ __forceinline__ void issue_next() {
    if (nleft == 0) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int rho = 8 * j + (lane >> 3);
      const int row = min(32 * (wave + MA_WAVES * ni) + (KEYMAP ? ma_key_of_row(rho) : rho), row_max);
      const int col = min(64 * nu + 8 * ((lane & 7) ^ ((rho >> 1) & 7)), ncol - 8);
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(base + ((unsigned)row * row_bytes + 2u * col)),
                                       (__attribute__((address_space(3))) void*)(ring + ns * MA_UNIT + j * 1024), 16, 0, 0);
    }
    --nleft;
    if (++nu == upt) { nu = 0; ++ni; }
    if (++ns == U) ns = 0;
  }
  __device__ __forceinline__ void start() {
    ni = nu = ns = 0;
    nleft = ntw * upt;
    for (int k = 0; k < U; ++k) issue_next();
  }
  template <int N>
  __device__ __forceinline__ void unit(f32x16& acc, const int slot, const int u) const {
    bf16x8 a[N], b[N];
    const unsigned bu = b_addr + 128 * u;
#pragma unroll
    for (int ks = 0; ks < N; ++ks) {
      a[ks] = ma_lds128<0>(a_addr[ks] + slot * MA_UNIT);
      if (ks == 0) b[ks] = ma_lds128<0>(bu);
      if (ks == 1) b[ks] = ma_lds128<32>(bu);
      if (ks == 2) b[ks] = ma_lds128<64>(bu);
      if (ks == 3) b[ks] = ma_lds128<96>(bu);
    }
#pragma unroll
    for (int ks = 0; ks < N; ++ks) {
      __builtin_amdgcn_sched_barrier(0);
      // LDS returns in order: all but the reads of the later k-steps have arrived (the waits take the fragments as
      // operands so that no MFMA moves above its wait)
      if (N - 1 - ks == 3) asm volatile("s_waitcnt lgkmcnt(6)" : "+v"(a[ks]), "+v"(b[ks])::"memory");
      if (N - 1 - ks == 2) asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(a[ks]), "+v"(b[ks])::"memory");
      if (N - 1 - ks == 1) asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(a[ks]), "+v"(b[ks])::"memory");
      if (N - 1 - ks == 0) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a[ks]), "+v"(b[ks])::"memory");
      __builtin_amdgcn_sched_barrier(0);
      acc = BMHRL_MFMA16(a[ks], b[ks], acc, 0, 0, 0);
    }
  }
  __device__ __forceinline__ void run(f32x16 (&acc)[MA_NT]) {
    const int G = ntw * upt;
    int g = 0, slot = 0;
#pragma unroll
    for (int i = 0; i < MA_NT; ++i) {
      if (i < ntw) {
        for (int u = 0; u < upt; ++u) {
          ma_wait_units(min(U - 1, G - g - 1));              // units g+1 .. are younger than unit g: it has landed
          __builtin_amdgcn_sched_barrier(0);
          const int n = u == upt - 1 ? ks_last : 4;
          if (n == 4) unit<4>(acc[i], slot, u);
          else if (n == 3) unit<3>(acc[i], slot, u);
          else if (n == 2) unit<2>(acc[i], slot, u);
          else unit<1>(acc[i], slot, u);
          __builtin_amdgcn_sched_barrier(0);                 // (the unit ended in lgkmcnt(0): its slot may be refilled)
          issue_next();
          ++g;
          if (++slot == U) slot = 0;
        }
      }
    }
  }
};

template <bool BWD>
__global__ __launch_bounds__(MA_THREADS) void mem_attn_kernel(const MemAttnArgs p) {
  __shared__ __attribute__((aligned(1024))) char lds[MA_LDS];                  // (the map: above)
  bf16_t* const Xs = reinterpret_cast<bf16_t*>(lds);                            // X rows; later the output image
  bf16_t* const Es = reinterpret_cast<bf16_t*>(lds + ma_es_off(p.Skp));         // P / dS rows [q][key]
  float (*const red)[32][2] = reinterpret_cast<float (*)[32][2]>(lds + MA_LDS - MA_RED);
  const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)lds;
  // workgroups are dealt round-robin over the 8 XCDs (private L2s).  All heads of a sample -- and the same sample of the other
  // fusion stack (b2 % nb) -- stream the SAME memory: give them block ids that differ by multiples of 8 so that one L2 fetches
  // it once (with the plain order the four heads of a sample sit on four XCDs: the memory came out of the Infinity Cache 4 x)
  int b2, hd;
  if (p.xcd_map) {
    const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
    hd = idx % p.H;
    b2 = xcd + 8 * (idx / p.H);
  } else {
    b2 = blockIdx.x / p.H;
    hd = blockIdx.x % p.H;
  }
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r32 = lane & 31, hh = lane >> 5;
  const int dm = p.dm, ldxs = dm + MA_PAD, ldes = p.Skp + MA_PAD;
  const int nt = (p.Sk + 31) / 32;
  const bf16_t* __restrict__ memb = p.mem + (long)(b2 % p.nb) * p.mem_sb;
  const bf16_t* __restrict__ memt = p.memT + (long)(b2 % p.nb) * p.memT_sb;

  // ---- pass 1, the stream: the rows of the memory, 64 columns of dm per unit (dm % 64 == 32: two k-steps in the last one).
  // Its first units are under way while X is staged.
  MaStream<true> s1;
  s1.base = reinterpret_cast<const char*>(memb); s1.row_bytes = 2u * dm; s1.ncol = dm; s1.row_max = p.Sk - 1;
  s1.ntw = (nt - wave + MA_WAVES - 1) / MA_WAVES; s1.upt = (dm + 63) / 64; s1.ks_last = dm / 16 - 4 * (s1.upt - 1);
  s1.U = ma_units1(dm);
  s1.wave = wave; s1.lane = lane;
  s1.ring = lds + ma_xs_bytes(dm) + wave * s1.U * MA_UNIT;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks)
    s1.a_addr[ks] = lds0 + ma_xs_bytes(dm) + wave * s1.U * MA_UNIT + r32 * 128 + (((2 * ks + hh) ^ ((r32 >> 1) & 7)) << 4);
  s1.b_addr = lds0 + (r32 * ldxs + 8 * hh) * 2;
  s1.start();

  // ---- X rows -> LDS (rows >= L zero)
  {
    const int cpr = dm / 8;
    for (int c = threadIdx.x; c < 32 * cpr; c += MA_THREADS) {
      const int row = c / cpr, ch = c % cpr;
      bf16x8 v = zero_bf16x8();
      if (row < p.L) v = *reinterpret_cast<const bf16x8*>(p.X + ((long)b2 * p.L + row) * p.ldx + hd * dm + ch * 8);
      *reinterpret_cast<bf16x8*>(Xs + row * ldxs + ch * 8) = v;
    }
  }
  __syncthreads();

  // ---- pass 1: this wave's key tiles (rows past the memory: clamped by the stream, masked below)
  f32x16 acc[MA_NT];
#pragma unroll
  for (int i = 0; i < MA_NT; ++i) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  }
  s1.run(acc);
  // this lane: query r32; register r of tile i: key 32 (wave + MA_WAVES i) + 8 hh + (r & 7) + 16 (r >> 3)
  const int q = r32;
  const uint8_t* mrow = p.mask ? p.mask + (long)b2 * p.mask_sb : nullptr;
  bf16_t* pd = p.PD + ((long)b2 * p.L + (q < p.L ? q : 0)) * p.pd_row + hd * p.Skp;
  if constexpr (!BWD) {
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < MA_NT; ++i) {
      const int k0 = 32 * (wave + MA_WAVES * i) + 8 * hh;
      if (wave + MA_WAVES * i < nt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = k0 + (r & 7) + 16 * (r >> 3);
          float s = acc[i][r] * p.scale;
          if (key >= p.Sk) s = -INFINITY;
          else if (mrow && !mrow[key]) s = NEG_MASK;
          acc[i][r] = s;
          m = fmaxf(m, s);
        }
      }
    }
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    if (hh == 0) red[wave][q][0] = m;
    __syncthreads();
    m = red[0][q][0];
#pragma unroll
    for (int w = 1; w < MA_WAVES; ++w) m = fmaxf(m, red[w][q][0]);
    float l = 0.f;
#pragma unroll
    for (int i = 0; i < MA_NT; ++i)
      if (wave + MA_WAVES * i < nt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          acc[i][r] = __expf(acc[i][r] - m);
          l += acc[i][r];
        }
      }
    l += __shfl_xor(l, 32, 64);
    if (hh == 0) red[wave][q][1] = l;
    __syncthreads();
    float lsum = 0.f;
#pragma unroll
    for (int w = 0; w < MA_WAVES; ++w) lsum += red[w][q][1];
    const float inv = 1.f / lsum;
#pragma unroll
    for (int i = 0; i < MA_NT; ++i)
      if (wave + MA_WAVES * i < nt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] *= inv;
      }
  } else {
    // P in the layout of the accumulators, delta = sum_k P dP over all keys, dS
    float delta = 0.f;
    bf16x8 pf[MA_NT][2];
#pragma unroll
    for (int i = 0; i < MA_NT; ++i) {
      pf[i][0] = pf[i][1] = zero_bf16x8();
      const int k0 = 32 * (wave + MA_WAVES * i) + 8 * hh;
      if (wave + MA_WAVES * i < nt && q < p.L) {
        if (k0 < p.Skp) pf[i][0] = *reinterpret_cast<const bf16x8*>(pd + k0);
        if (k0 + 16 < p.Skp) pf[i][1] = *reinterpret_cast<const bf16x8*>(pd + k0 + 16);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) delta = fmaf((float)pf[i][r >> 3][r & 7], acc[i][r], delta);
    }
    delta += __shfl_xor(delta, 32, 64);
    if (hh == 0) red[wave][q][0] = delta;
    __syncthreads();
    delta = 0.f;
#pragma unroll
    for (int w = 0; w < MA_WAVES; ++w) delta += red[w][q][0];
#pragma unroll
    for (int i = 0; i < MA_NT; ++i) {
      const int k0 = 32 * (wave + MA_WAVES * i) + 8 * hh;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = k0 + (r & 7) + 16 * (r >> 3);
        float v = p.scale * (float)pf[i][r >> 3][r & 7] * (acc[i][r] - delta);
        if (key >= p.Sk || (mrow && !mrow[min(key, p.Sk - 1)])) v = 0.f;      // masked_fill: no gradient reaches a masked score
        acc[i][r] = v;
      }
    }
  }
  // E (P or dS) -> bf16: HBM (slot of the interleaved buffer) and the LDS image of pass 2
  bf16_t* eg = pd + (BWD ? p.pd_slot : 0);
#pragma unroll
  for (int i = 0; i < MA_NT; ++i) {
    const int k0 = 32 * (wave + MA_WAVES * i) + 8 * hh;
    if (wave + MA_WAVES * i < nt) {
      bf16x8 e0, e1;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        e0[j] = (bf16_t)acc[i][j];
        e1[j] = (bf16_t)acc[i][8 + j];
      }
      if (k0 < p.Skp) *reinterpret_cast<bf16x8*>(Es + q * ldes + k0) = e0;
      if (k0 + 16 < p.Skp) *reinterpret_cast<bf16x8*>(Es + q * ldes + k0 + 16) = e1;
      if (q < p.L) {
        if (k0 < p.Skp) *reinterpret_cast<bf16x8*>(eg + k0) = e0;
        if (k0 + 16 < p.Skp) *reinterpret_cast<bf16x8*>(eg + k0 + 16) = e1;
      }
    }
  }
  // keys between Skp and the next multiple of 16 (pass 2 walks whole 16-key steps): zero in the image
  {
    const int kend = (p.Sk + 15) & ~15;
    for (int c = threadIdx.x; c < 32 * (kend - p.Skp); c += MA_THREADS) Es[(c / (kend - p.Skp)) * ldes + p.Skp + c % (kend - p.Skp)] = (bf16_t)0.f;
  }
  __syncthreads();                                  // E image complete; every wave is done with Xs

  // ---- pass 2: Y^T[d][q] = sum_key memT[d][key] E[q][key], the d-tiles dealt to the waves
  // The stream: the rows of memT, 64 keys per unit; whole 16-key steps up to Sk (columns in [Sk, ldt) are zero, loads stop
  // at ldt).  Its ring lies over Xs, so the output tiles stay in the accumulators until every wave has left the stream.
  const int nks = (p.Sk + 15) / 16;
  MaStream<false> s2;
  s2.base = reinterpret_cast<const char*>(memt); s2.row_bytes = 2u * p.ldt; s2.ncol = p.ldt; s2.row_max = dm - 1;
  s2.ntw = (dm / 32 - wave + MA_WAVES - 1) / MA_WAVES; s2.upt = (nks + 3) / 4; s2.ks_last = nks - 4 * (s2.upt - 1);
  s2.U = ma_units2(p.Skp);
  s2.wave = wave; s2.lane = lane;
  s2.ring = lds + wave * s2.U * MA_UNIT;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) s2.a_addr[ks] = lds0 + wave * s2.U * MA_UNIT + r32 * 128 + (((2 * ks + hh) ^ ((r32 >> 1) & 7)) << 4);
  s2.b_addr = lds0 + ma_es_off(p.Skp) + (r32 * ldes + 8 * hh) * 2;
  s2.start();
#pragma unroll
  for (int i = 0; i < MA_NT; ++i) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  }
  s2.run(acc);
  __syncthreads();                                  // every wave is done with its ring: Xs takes the output image
#pragma unroll
  for (int i = 0; i < MA_NT; ++i) {
    const int dt = wave + MA_WAVES * i;
    if (dt < dm / 32) {
#pragma unroll
      for (int r = 0; r < 16; ++r) Xs[q * ldxs + dt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh] = (bf16_t)acc[i][r];
    }
  }
  __syncthreads();
  {
    const int cpr = dm / 8;
    for (int c = threadIdx.x; c < 32 * cpr; c += MA_THREADS) {
      const int row = c / cpr, ch = c % cpr;
      if (row < p.L)
        *reinterpret_cast<bf16x8*>(p.Y + ((long)b2 * p.L + row) * p.ldy + hd * dm + ch * 8) = *reinterpret_cast<const bf16x8*>(Xs + row * ldxs + ch * 8);
    }
  }
}

// fp32 (B * Sk, dm) -> bf16 row-major copy (B * Sk, dm) AND the per-sample transposed copy (B, dm, ldt), one pass
__global__ void cast_memory_kernel(const float* __restrict__ x, bf16_t* __restrict__ y, bf16_t* __restrict__ yt, int Sk, int dm, int ldt) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z, k0 = blockIdx.y * 32, d0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;            // 32 x 8
  for (int r = ty; r < 32; r += 8) {
    const int key = k0 + r;
    float v = 0.f;
    if (key < Sk) {
      v = x[((long)b * Sk + key) * dm + d0 + tx];
      y[((long)b * Sk + key) * dm + d0 + tx] = (bf16_t)v;
    }
    tile[r][tx] = v;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int key = k0 + tx;
    if (key < ldt) yt[((long)b * dm + d0 + r) * ldt + key] = (bf16_t)tile[tx][r];      // (keys in [Sk, ldt): zero)
  }
}

bool ma_aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

}  // namespace

extern "C" int bmhrl_memory_attention_ok(int32_t L, int32_t Sk, int32_t dm) {
  return L >= 1 && L <= 32 && Sk >= 1 && Sk <= MA_MAXK && dm >= 32 && dm <= MA_MAXD && dm % 32 == 0 &&
         ma_units1(dm) >= 1 && ma_units2((Sk + 7) & ~7) >= 1;          // (both streams have a ring: see the LDS map)
}

extern "C" int bmhrl_cast_memory(const float* x, void* y, void* y_t, int32_t B, int32_t Sk, int32_t dm, int32_t ldt,
                                 bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG(x && y && y_t && B > 0 && Sk > 0 && dm > 0 && dm % 32 == 0 && ldt >= Sk && ldt % 8 == 0 && B <= 65535);
  dim3 grid((unsigned)(dm / 32), (unsigned)((ldt + 31) / 32), (unsigned)B), block(256);
  hipLaunchKernelGGL(cast_memory_kernel, grid, block, 0, (hipStream_t)stream, x, (bf16_t*)y, (bf16_t*)y_t, Sk, dm, ldt);
  return hip_status(hipGetLastError());
}

extern "C" int bmhrl_memory_attention(int32_t backward, const void* X, int64_t ldx, const void* mem, int64_t mem_sb,
                                      const void* mem_t, int64_t mem_t_sb, int32_t ldt, void* PD, int64_t pd_row,
                                      int64_t pd_slot, void* Y, int64_t ldy, const uint8_t* mask, int64_t mask_sb, int32_t n_mem,
                                      int32_t B2, int32_t H, int32_t L, int32_t Sk, int32_t dm, float scale,
                                      bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG(X && mem && mem_t && PD && Y && B2 > 0 && H > 0 && n_mem > 0 && bmhrl_memory_attention_ok(L, Sk, dm));
  const int Skp = (Sk + 7) & ~7;
  BMHRL_CHECK_ARG(ldx % 8 == 0 && ldy % 8 == 0 && pd_row % 8 == 0 && pd_slot % 8 == 0 && ldt % 8 == 0 && ldt >= ((Sk + 15) & ~15));
  BMHRL_CHECK_ARG(mem_sb % 8 == 0 && mem_t_sb % 8 == 0 && pd_row >= (int64_t)H * Skp && (long)B2 * H < (1l << 31));
  BMHRL_CHECK_ARG(ma_aligned16(X) && ma_aligned16(mem) && ma_aligned16(mem_t) && ma_aligned16(PD) && ma_aligned16(Y));
  MemAttnArgs a;
  a.X = (const bf16_t*)X; a.ldx = ldx; a.mem = (const bf16_t*)mem; a.mem_sb = mem_sb;
  a.memT = (const bf16_t*)mem_t; a.memT_sb = mem_t_sb; a.ldt = ldt;
  a.PD = (bf16_t*)PD; a.pd_row = pd_row; a.pd_slot = pd_slot; a.Y = (bf16_t*)Y; a.ldy = ldy;
  a.mask = mask; a.mask_sb = mask_sb; a.nb = n_mem; a.H = H; a.L = L; a.Sk = Sk; a.Skp = Skp; a.dm = dm; a.scale = scale;
  static const bool plain = getenv("BMHRL_MEMATTN_PLAINMAP") != nullptr;      // (A/B switch)
  a.xcd_map = (B2 % 8 == 0 && !plain) ? 1 : 0;
  dim3 grid((unsigned)(B2 * H)), block(MA_THREADS);
  if (backward) hipLaunchKernelGGL(mem_attn_kernel<true>, grid, block, 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(mem_attn_kernel<false>, grid, block, 0, (hipStream_t)stream, a);
  return hip_status(hipGetLastError());
}
