// Training of the segment critic (LSTM(4) -> AReLU -> GRU(2) -> AReLU -> Linear(600 -> 1)) for gfx950, fp32 throughout like
// the inference kernels of critic.hip.  Layer by layer, eagerly:
//   forward  : bmhrl_gemm_f32 (input projection) + one bmhrl_rnn_step_train per (layer, t): the recurrent product on the f32
//              matrix pipe, the cell equations of rnn_step_kernel, and everything the backward needs kept (raw h_t, the
//              shifted sequence H_prev, c_t, the gate activations, the GRU's W_hn h + b_hn)
//   backward : one bmhrl_rnn_bwd_step per (layer, t), t descending -- the launch of step t first finishes step t + 1 (the
//              carried dh = dA_h[t + 1] . W_hh on the f32 matrix pipe) and then runs the cell equations of step t;
//              after the time loop of a layer the batched products dX / dW_ih / dW_hh (bmhrl_gemm_f32_nn), the bias
//              column sums and the AReLU scalar sums
//   head     : bmhrl_critic_head_loss -- score, masked BCE-with-logits, ds, dy2, dlin_w, dlin_b in one launch
// Every sum has a fixed order (k-ordered MFMA chains, partial sums added in a fixed order, no float atomics): two runs of
// the same step agree bit for bit.  Zero initial state: h_{-1} = c_{-1} = 0.
//
// The two step kernels share one shape: a block owns 16 hidden units x 16 batch rows and runs 16 waves that split the
// product over (gate, k) on v_mfma_f32_16x16x4_f32 (A: 16 weight rows, B: 16 batch rows).  Lane (r = lane & 15, q = lane >> 4)
// holds k = 16 s + 4 q + e of step s for MFMA e on both operands.  No operand is shared between the waves of a block, so
// nothing is staged in LDS: k is tiled over the waves, every weight byte is read once per block straight from global
// memory (L2 / Infinity Cache: a layer's W_hh is 5.76 MB), and only the 16 x 16 partial tiles go through LDS.  A wave
// requests all of its operand pieces (<= WAVE_STEPS steps) before its first MFMA: one memory latency per launch.
#include "common.h"
#include "../../include/bmhrl_hip.h"

namespace {

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float arelu_(float x, float alpha, float beta) {
  return x > 0.f ? x * (1.f + sigmoidf_(beta)) : x * fminf(fmaxf(alpha, 0.01f), 0.99f);
}
// d arelu(x) / dx
__device__ __forceinline__ float arelu_slope_(float x, float alpha, float beta) {
  return x > 0.f ? 1.f + sigmoidf_(beta) : (x < 0.f ? fminf(fmaxf(alpha, 0.01f), 0.99f) : 0.f);
}
__device__ __forceinline__ f32x4 mfma4_(const f32x4 a, const f32x4 b, f32x4 acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], b[0], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], b[1], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], b[2], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], b[3], acc, 0, 0, 0);
  return acc;
}

constexpr int MAXH = 640;      // as critic.hip
// 16-column steps of one wave: the forward splits k <= MAXH over 4 waves per gate, the backward k <= 4 MAXH over 16 waves
constexpr int WAVE_STEPS = (MAXH / 16 + 3) / 4;
static_assert(WAVE_STEPS == (4 * MAXH / 16 + 15) / 16, "both step kernels hold WAVE_STEPS steps per wave");

// ---------------------------------------------------------------------------------------------- training forward step
// Sequence buffers, row b*L + t:  h_seq (B*L, H) raw h_t;  hprev_seq (B*L, H) = h_{t-1}, zero at t = 0 (the step reads its
// row t and writes row t + 1: it is the H_prev of dW_hh as well);  c_seq (LSTM);  gate_seq (B*L, GATES*H) the activations
// i,f,g,o / r,z,n;  hn_seq (GRU) = W_hn h_{t-1} + b_hn;  y_seq = AReLU(h_t) when the layer ends a stack.
// Wave (k quarter, gate) multiplies the 16 rows of its gate of W_hh over a quarter of k; the four partial tiles of a gate
// are added as (0 + 1) + (2 + 3); the association with xproj and the biases is rnn_step_kernel's.
template <int GATES>
__global__ __launch_bounds__(1024) void rnn_step_train_kernel(const float* __restrict__ xproj, const float* __restrict__ whh,
                                                               const float* __restrict__ bhh, float* __restrict__ h_seq,
                                                               float* hprev_seq, float* __restrict__ c_seq,
                                                               float* __restrict__ gate_seq, float* __restrict__ hn_seq,
                                                               float* __restrict__ y_seq, const float* __restrict__ ar_alpha,
                                                               const float* __restrict__ ar_beta, int B, int L, int H, int t) {
  __shared__ float sh_g[4][4][16][17];                                 // [k quarter][gate][unit][batch row]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r = lane & 15, kq = lane >> 4;
  const int part = wave >> 2, gate = wave & 3;
  const int u0 = blockIdx.x * 16, b0 = blockIdx.y * 16;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (t > 0 && gate < GATES) {                                         // uniform for the wave
    const int nsteps = (H + 15) / 16, per = (nsteps + 3) / 4;
    const int s0 = part * per, n = min(nsteps, s0 + per) - s0;
    const bool u_ok = u0 + r < H, b_ok = b0 + r < B;
    const float* wp = whh + ((long)gate * H + (u_ok ? u0 + r : 0)) * H;
    const float* hp = hprev_seq + ((long)(b_ok ? b0 + r : 0) * L + t) * H;
    f32x4 w[WAVE_STEPS], a[WAVE_STEPS];
#pragma unroll
    for (int i = 0; i < WAVE_STEPS; ++i) {                             // every load of the wave is requested before the first MFMA
      const int k = 16 * (s0 + i) + 4 * kq, kc = max(min(k, H - 4), 0);  // H % 4 == 0: a lane's four k are in or out together
      const bool live = i < n && k < H;
      w[i] = live && u_ok ? *reinterpret_cast<const f32x4*>(wp + kc) : f32x4{0.f, 0.f, 0.f, 0.f};
      a[i] = live && b_ok ? *reinterpret_cast<const f32x4*>(hp + kc) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int i = 0; i < WAVE_STEPS; ++i)
      if (i < n) acc = mfma4_(w[i], a[i], acc);                        // uniform
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) sh_g[part][gate][4 * kq + i][r] = acc[i];   // accumulator: unit 4 q + i, batch row r
  __syncthreads();
  if (tid < 256) {
    const int ul = tid >> 4, bl = tid & 15, u = u0 + ul, b = b0 + bl;
    if (u < H && b < B) {
      const long row = (long)b * L + t;
      const float* xp = xproj + row * (GATES * H);
      float* ga = gate_seq + row * (GATES * H);
      float hh[GATES];
#pragma unroll
      for (int g = 0; g < GATES; ++g) {
        hh[g] = (sh_g[0][g][ul][bl] + sh_g[1][g][ul][bl]) + (sh_g[2][g][ul][bl] + sh_g[3][g][ul][bl]);
        if (GATES == 3) hh[g] += bhh[g * H + u];
      }
      float hn;
      if (GATES == 4) {
        const float gi = sigmoidf_(xp[u] + hh[0]);
        const float gf = sigmoidf_(xp[H + u] + hh[1]);
        const float gg = tanhf(xp[2 * H + u] + hh[2]);
        const float go = sigmoidf_(xp[3 * H + u] + hh[GATES - 1]);
        const float c = gf * (t > 0 ? c_seq[(row - 1) * H + u] : 0.f) + gi * gg;
        c_seq[row * H + u] = c;
        ga[u] = gi; ga[H + u] = gf; ga[2 * H + u] = gg; ga[3 * H + u] = go;
        hn = go * tanhf(c);
      } else {
        const float gr = sigmoidf_(xp[u] + hh[0]);
        const float gz = sigmoidf_(xp[H + u] + hh[1]);
        const float gn = tanhf(xp[2 * H + u] + gr * hh[2]);
        ga[u] = gr; ga[H + u] = gz; ga[2 * H + u] = gn;
        hn_seq[row * H + u] = hh[2];
        hn = (1.f - gz) * gn + gz * (t > 0 ? hprev_seq[row * H + u] : 0.f);
      }
      h_seq[row * H + u] = hn;
      if (t == 0) hprev_seq[row * H + u] = 0.f;
      if (t + 1 < L) hprev_seq[(row + 1) * H + u] = hn;
      if (ar_alpha) y_seq[row * H + u] = arelu_(hn, ar_alpha[0], ar_beta[0]);
    }
  }
}

// ---------------------------------------------------------------------------------------------- backward cell step
//  1. (t + 1 < L)  carried dh[b][u] = sum_k dA_h[t + 1][b][k] * W_hh[k][u], k < GATES * H: the 16 waves split k (A = W_hh^T:
//     row = unit, B = dA_h^T: column = batch row).  Lane (r, q) reads W_hh[16 s + 4 q + e][u0 + r] (the 16 lanes of a q cover
//     64 contiguous bytes of a weight row: W_hh needs no transposed copy) and the 16 bytes dA_h[b0 + r][16 s + 4 q ..].  The
//     16 partial tiles are added in wave order.
//  2. 256 threads run the cell equations of step t for their (unit, batch row) and write dA_x[t] / dA_h[t] and the
//     element-wise carry (LSTM: dc . f, GRU: dh . z) that the same thread reads back in the launch of step t - 1.
template <int GATES>
__global__ __launch_bounds__(1024) void rnn_bwd_step_kernel(const float* __restrict__ whh, const float* __restrict__ dy,
                                                             const float* __restrict__ h_seq, const float* __restrict__ c_seq,
                                                             const float* __restrict__ gate_seq, const float* __restrict__ hn_seq,
                                                             float* __restrict__ carry, float* dax /* LSTM: == dah */,
                                                             float* dah, const float* __restrict__ ar_alpha,
                                                             const float* __restrict__ ar_beta, int B, int L, int H, int t) {
  __shared__ float sh_p[16][16][17];                                   // [wave][unit][batch row]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r = lane & 15, kq = lane >> 4;
  const int u0 = blockIdx.x * 16, b0 = blockIdx.y * 16;
  const int GH = GATES * H;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (t + 1 < L) {                                                     // uniform
    const int nsteps = (GH + 15) / 16, per = (nsteps + 15) / 16;
    const int s0 = wave * per, n = min(nsteps, s0 + per) - s0;
    const bool u_ok = u0 + r < H, b_ok = b0 + r < B;
    const float* wp = whh + (u_ok ? u0 + r : 0);
    const float* ap = dah + ((long)(b_ok ? b0 + r : 0) * L + t + 1) * GH;
    f32x4 w[WAVE_STEPS], a[WAVE_STEPS];
#pragma unroll
    for (int i = 0; i < WAVE_STEPS; ++i) {                             // every load of the wave is requested before the first MFMA
      const int k = 16 * (s0 + i) + 4 * kq, kc = max(min(k, GH - 4), 0);  // GH % 4 == 0: a lane's four k are in or out together
      const bool live = i < n && k < GH;
      a[i] = live && b_ok ? *reinterpret_cast<const f32x4*>(ap + kc) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int e = 0; e < 4; ++e) w[i][e] = live && u_ok ? wp[(long)(kc + e) * H] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < WAVE_STEPS; ++i)
      if (i < n) acc = mfma4_(w[i], a[i], acc);                        // uniform
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) sh_p[wave][4 * kq + i][r] = acc[i];      // accumulator: unit 4 q + i, batch row r
  __syncthreads();
  if (tid < 256) {
    const int ul = tid >> 4, bl = tid & 15, u = u0 + ul, b = b0 + bl;
    if (u < H && b < B) {
      float dh = 0.f;
#pragma unroll
      for (int w = 0; w < 16; ++w) dh += sh_p[w][ul][bl];
      const long row = (long)b * L + t;
      const float cin = t + 1 < L ? carry[(long)b * H + u] : 0.f;
      const float hv = h_seq[row * H + u];
      float dyv = dy[row * H + u];
      if (ar_alpha) dyv *= arelu_slope_(hv, ar_alpha[0], ar_beta[0]);
      const float* ga = gate_seq + row * GH;
      float* ox = dax + row * GH;
      if (GATES == 4) {
        dh = dyv + dh;
        const float gi = ga[u], gf = ga[H + u], gg = ga[2 * H + u], go = ga[3 * H + u];
        const float tc = tanhf(c_seq[row * H + u]);
        const float cp = t > 0 ? c_seq[(row - 1) * H + u] : 0.f;
        const float d_o = dh * tc;
        const float dc = cin + dh * go * (1.f - tc * tc);
        carry[(long)b * H + u] = dc * gf;
        ox[u] = dc * gg * (gi * (1.f - gi));
        ox[H + u] = dc * cp * (gf * (1.f - gf));
        ox[2 * H + u] = dc * gi * (1.f - gg * gg);
        ox[3 * H + u] = d_o * (go * (1.f - go));
      } else {
        dh = dyv + (cin + dh);
        const float gr = ga[u], gz = ga[H + u], gn = ga[2 * H + u];
        const float hp = t > 0 ? h_seq[(row - 1) * H + u] : 0.f;
        const float dan = dh * (1.f - gz) * (1.f - gn * gn);
        const float dar = dan * hn_seq[row * H + u] * (gr * (1.f - gr));
        const float daz = dh * (hp - gn) * (gz * (1.f - gz));
        carry[(long)b * H + u] = dh * gz;
        ox[u] = dar; ox[H + u] = daz; ox[2 * H + u] = dan;
        float* oh = dah + row * GH;
        oh[u] = dar; oh[H + u] = daz; oh[2 * H + u] = dan * gr;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------- batched products
// C[M,N] = op(A) . B with B (K, N) row-major ("k-major": the layout of the weights and of the activation sequences as the
// backward meets them), A (M, K) row-major (AK = false, K % 4 == 0) or (K, M) row-major (AK = true, any K).  One wave per
// 32x32 tile on v_mfma_f32_32x32x2_f32 (a k-ascending fmaf chain per element), 2x2 waves per block; lane (r32, h) feeds
// k + h and k + 2 + h of every group of four.  The main loop takes 16 k at a time with all 16 loads ahead of the 8 MFMAs.
template <bool AK>
__global__ __launch_bounds__(256) void gemm_f32_nn_kernel(const float* __restrict__ A, long lda, const float* __restrict__ Bm,
                                                           long ldb, float* __restrict__ C, long ldc, int M, int N, int K) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r32 = lane & 31, h = lane >> 5;
  const int m0 = blockIdx.y * 64 + (wave >> 1) * 32, n0 = blockIdx.x * 64 + (wave & 1) * 32;
  if (m0 >= M || n0 >= N) return;
  const int m = min(m0 + r32, M - 1), n = min(n0 + r32, N - 1);
  const float* bp = Bm + n;
  const float* ap = AK ? A + m : A + (long)m * lda;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  int k = 0;
  for (; k + 16 <= K; k += 16) {
    float a0[4], a1[4], w0[4], w1[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k0 = k + 4 * j + h, k1 = k0 + 2;
      if (AK) {
        a0[j] = ap[(long)k0 * lda];
        a1[j] = ap[(long)k1 * lda];
      } else {
        const f32x4 a = *reinterpret_cast<const f32x4*>(ap + k + 4 * j);
        a0[j] = h ? a[1] : a[0];
        a1[j] = h ? a[3] : a[2];
      }
      w0[j] = bp[(long)k0 * ldb];
      w1[j] = bp[(long)k1 * ldb];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[j], w0[j], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[j], w1[j], acc, 0, 0, 0);
    }
  }
  for (; k < K; k += 4) {                                              // tail: fewer than 16 k left, element-wise guards
    const int k0 = k + h, k1 = k + 2 + h;
    float a0, a1;
    if (AK) {
      a0 = k0 < K ? ap[(long)k0 * lda] : 0.f;
      a1 = k1 < K ? ap[(long)k1 * lda] : 0.f;
    } else {
      const f32x4 a = *reinterpret_cast<const f32x4*>(ap + k);
      a0 = h ? a[1] : a[0];
      a1 = h ? a[3] : a[2];
    }
    const float w0 = k0 < K ? bp[(long)k0 * ldb] : 0.f;
    const float w1 = k1 < K ? bp[(long)k1 * ldb] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, w0, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, w1, acc, 0, 0, 0);
  }
  if (n0 + r32 < N) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int mm = m0 + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (mm < M) C[(long)mm * ldc + n0 + r32] = acc[r];
    }
  }
}

// ---------------------------------------------------------------------------------------------- reductions
// Column sums of dA_x (blockIdx.y = 0) and dA_h (1) over the B*L rows: 32 columns x 32 row groups per block; a thread adds
// the rows of its group in ascending order, the 32 partials are added in group order.
__global__ __launch_bounds__(1024) void rnn_bias_grad_kernel(const float* __restrict__ dax, const float* __restrict__ dah,
                                                              float* __restrict__ dbx, float* __restrict__ dbh, long rows, int N) {
  __shared__ float sh[32][33];
  const float* src = blockIdx.y == 0 ? dax : dah;
  float* dst = blockIdx.y == 0 ? dbx : dbh;
  const int c = threadIdx.x & 31, g = threadIdx.x >> 5, col = blockIdx.x * 32 + c;
  float acc = 0.f;
  if (col < N)
    for (long r = g; r < rows; r += 32) acc += src[r * N + col];
  sh[g][c] = acc;
  __syncthreads();
  if (threadIdx.x < 32 && col < N) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i) s += sh[i][c];
    dst[col] = s;
  }
}

// AReLU scalars: pos = sum dy relu(h), neg = sum dy relu(-h).  ARELU_PARTS blocks each add a strided share in a fixed
// order (block_sum: shuffle tree + wave order); the finish adds the parts in order.
constexpr int ARELU_PARTS = 64;
__global__ __launch_bounds__(256) void arelu_grad_partial_kernel(const float* __restrict__ dy, const float* __restrict__ h,
                                                                  float* __restrict__ partial, long n) {
  __shared__ float red[16];
  float pos = 0.f, neg = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)ARELU_PARTS * 256) {
    const float g = dy[i], x = h[i];
    pos += g * fmaxf(x, 0.f);
    neg += g * fmaxf(-x, 0.f);
  }
  pos = block_sum(pos, red);
  neg = block_sum(neg, red);
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = pos;
    partial[ARELU_PARTS + blockIdx.x] = neg;
  }
}
__global__ void arelu_grad_finish_kernel(const float* __restrict__ partial, const float* __restrict__ alpha,
                                         const float* __restrict__ beta, float* __restrict__ dalpha, float* __restrict__ dbeta) {
  if (threadIdx.x != 0) return;
  float pos = 0.f, neg = 0.f;
  for (int i = 0; i < ARELU_PARTS; ++i) { pos += partial[i]; neg += partial[ARELU_PARTS + i]; }
  const float sg = sigmoidf_(beta[0]), a = alpha[0];
  dbeta[0] = pos * (sg * (1.f - sg));
  dalpha[0] = (a >= 0.01f && a <= 0.99f) ? -neg : 0.f;             // torch.clamp passes the gradient at both ends
}

// ---------------------------------------------------------------------------------------------- head + loss
// One block of 16 waves.  With labels: s = lin_w . y2 + lin_b, the masked BCE-with-logits (positive weight pw) and its ds;
// without: ds = ds_in (the gradient of the score from autograd).  Then dy2 = ds lin_w, dlin_w = sum ds y2, dlin_b = sum ds.
// Wave w takes the rows w, w + 16, ... in order and the per-wave sums are added in wave order.  For dlin_w / dy2 a thread
// owns four columns and one of HL_GROUPS row groups, adds its rows in ascending order, and the group partials are added
// in group order.
constexpr int HL_GROUPS = 6;                                           // 6 x (640 / 4) threads <= 1024
__global__ __launch_bounds__(1024) void critic_head_loss_kernel(const float* __restrict__ y2, const float* __restrict__ lw,
                                                                 const float* __restrict__ lb, const float* __restrict__ labels,
                                                                 const uint8_t* __restrict__ mask, float pw,
                                                                 const float* __restrict__ ds_in, float* __restrict__ score,
                                                                 float* __restrict__ loss, float* ds, float* __restrict__ dy2,
                                                                 float* __restrict__ dlw, float* __restrict__ dlb, long rows,
                                                                 int H) {
  __shared__ float red[16];
  __shared__ float sh_l[16], sh_d[16];
  __shared__ __attribute__((aligned(16))) float sh_w[HL_GROUPS][MAXH];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int nc4 = H / 4;
  float nm = 1.f;
  if (labels) {
    float cnt = 0.f;
    for (long r = tid; r < rows; r += 1024) cnt += mask[r] ? 1.f : 0.f;
    nm = block_sum(cnt, red);                                          // (a count: exact in any order)
  }
  float lsum = 0.f, dsum = 0.f;
  for (long row = wave; row < rows; row += 16) {
    float d;
    if (labels) {
      float acc = 0.f;
      for (int k = lane; k < H; k += 64) acc = fmaf(y2[row * H + k], lw[k], acc);   // critic_head_kernel's order: same bits
      const float s = wave_sum(acc) + lb[0];
      const float y = labels[row], mk = mask[row] ? 1.f : 0.f;
      const float l = (1.f - y) * s + (1.f + (pw - 1.f) * y) * (log1pf(expf(-fabsf(s))) + fmaxf(-s, 0.f));
      d = mk * (sigmoidf_(s) * (1.f - y + pw * y) - pw * y) / nm;
      lsum += mk * l;
      if (lane == 0 && score) score[row] = s;
    } else {
      d = ds_in[row];
    }
    dsum += d;
    if (lane == 0) ds[row] = d;
  }
  if (lane == 0) { sh_l[wave] = lsum; sh_d[wave] = dsum; }
  __syncthreads();                                                     // (also orders the ds stores before the reads below)
  if (tid == 0) {
    float l = 0.f, d = 0.f;
    for (int w = 0; w < 16; ++w) { l += sh_l[w]; d += sh_d[w]; }
    if (labels) loss[0] = l / nm;
    dlb[0] = d;
  }
  const int c4 = tid % nc4, grp = tid / nc4;
  if (grp < HL_GROUPS) {
    const f32x4 w = *reinterpret_cast<const f32x4*>(lw + 4 * c4);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (long row = grp; row < rows; row += HL_GROUPS) {
      const float d = ds[row];
      const f32x4 y = *reinterpret_cast<const f32x4*>(y2 + row * H + 4 * c4);
      acc[0] = fmaf(d, y[0], acc[0]); acc[1] = fmaf(d, y[1], acc[1]); acc[2] = fmaf(d, y[2], acc[2]); acc[3] = fmaf(d, y[3], acc[3]);
      *reinterpret_cast<f32x4*>(dy2 + row * H + 4 * c4) = f32x4{d * w[0], d * w[1], d * w[2], d * w[3]};
    }
    *reinterpret_cast<f32x4*>(&sh_w[grp][4 * c4]) = acc;
  }
  __syncthreads();
  if (tid < H) {
    float s = 0.f;
#pragma unroll
    for (int g = 0; g < HL_GROUPS; ++g) s += sh_w[g][tid];
    dlw[tid] = s;
  }
}

}  // namespace

#define S_(x) ((hipStream_t)(x))

extern "C" int bmhrl_rnn_step_train(int32_t gates, const float* xproj, const float* whh, const float* bhh, float* h_seq,
                                    float* hprev_seq, float* c_seq, float* gate_seq, float* hn_seq, float* y_seq,
                                    const float* arelu_alpha, const float* arelu_beta, int32_t B, int32_t L, int32_t H, int32_t t,
                                    bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG((gates == 3 || gates == 4) && xproj && whh && h_seq && hprev_seq && gate_seq && B > 0 && L > 0 && t >= 0 && t < L);
  BMHRL_CHECK_ARG(H > 0 && H <= MAXH && H % 4 == 0 && (gates == 3 ? (bhh != nullptr && hn_seq != nullptr) : c_seq != nullptr));
  BMHRL_CHECK_ARG((arelu_alpha == nullptr) == (arelu_beta == nullptr) && (arelu_alpha == nullptr || y_seq != nullptr));
  BMHRL_CHECK_ARG((((uintptr_t)whh | (uintptr_t)hprev_seq) & 15) == 0);
  dim3 grid((unsigned)((H + 15) / 16), (unsigned)((B + 15) / 16)), block(1024);
  if (gates == 4)
    hipLaunchKernelGGL(rnn_step_train_kernel<4>, grid, block, 0, S_(stream), xproj, whh, bhh, h_seq, hprev_seq, c_seq, gate_seq, hn_seq,
                       y_seq, arelu_alpha, arelu_beta, B, L, H, t);
  else
    hipLaunchKernelGGL(rnn_step_train_kernel<3>, grid, block, 0, S_(stream), xproj, whh, bhh, h_seq, hprev_seq, c_seq, gate_seq, hn_seq,
                       y_seq, arelu_alpha, arelu_beta, B, L, H, t);
  return hip_status(hipGetLastError());
}

extern "C" int bmhrl_rnn_bwd_step(int32_t gates, const float* whh, const float* dy, const float* h_seq, const float* c_seq,
                                  const float* gate_seq, const float* hn_seq, float* carry, float* dax, float* dah,
                                  const float* arelu_alpha, const float* arelu_beta, int32_t B, int32_t L, int32_t H, int32_t t,
                                  bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG((gates == 3 || gates == 4) && whh && dy && h_seq && gate_seq && carry && dax && B > 0 && L > 0 && t >= 0 && t < L);
  BMHRL_CHECK_ARG(H > 0 && H <= MAXH && H % 4 == 0 && (gates == 3 ? (hn_seq != nullptr && dah != nullptr) : c_seq != nullptr));
  BMHRL_CHECK_ARG((arelu_alpha == nullptr) == (arelu_beta == nullptr));
  if (gates == 4) dah = dax;                                           // the LSTM's dA_h is its dA_x: one buffer
  BMHRL_CHECK_ARG(((uintptr_t)dah & 15) == 0);
  dim3 grid((unsigned)((H + 15) / 16), (unsigned)((B + 15) / 16)), block(1024);
  if (gates == 4)
    hipLaunchKernelGGL(rnn_bwd_step_kernel<4>, grid, block, 0, S_(stream), whh, dy, h_seq, c_seq, gate_seq, hn_seq, carry, dax, dah,
                       arelu_alpha, arelu_beta, B, L, H, t);
  else
    hipLaunchKernelGGL(rnn_bwd_step_kernel<3>, grid, block, 0, S_(stream), whh, dy, h_seq, c_seq, gate_seq, hn_seq, carry, dax, dah,
                       arelu_alpha, arelu_beta, B, L, H, t);
  return hip_status(hipGetLastError());
}

extern "C" int bmhrl_gemm_f32_nn(const float* A, int64_t lda, int32_t a_kmajor, const float* Bm, int64_t ldb, float* C,
                                 int64_t ldc, int32_t M, int32_t N, int32_t K, bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG(A && Bm && C && M > 0 && N > 0 && K > 0 && ldb >= N && ldc >= N);
  BMHRL_CHECK_ARG(a_kmajor ? lda >= M : (lda >= K && K % 4 == 0 && lda % 4 == 0 && ((uintptr_t)A & 15) == 0));
  dim3 grid((unsigned)((N + 63) / 64), (unsigned)((M + 63) / 64)), block(256);
  if (a_kmajor)
    hipLaunchKernelGGL(gemm_f32_nn_kernel<true>, grid, block, 0, S_(stream), A, (long)lda, Bm, (long)ldb, C, (long)ldc, M, N, K);
  else
    hipLaunchKernelGGL(gemm_f32_nn_kernel<false>, grid, block, 0, S_(stream), A, (long)lda, Bm, (long)ldb, C, (long)ldc, M, N, K);
  return hip_status(hipGetLastError());
}

extern "C" int bmhrl_rnn_bias_grad(const float* dax, const float* dah, float* db_x, float* db_h, int64_t rows, int32_t N,
                                   bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG(dax && db_x && rows > 0 && N > 0 && (dah == nullptr) == (db_h == nullptr));
  dim3 grid((unsigned)((N + 31) / 32), dah ? 2u : 1u), block(1024);
  hipLaunchKernelGGL(rnn_bias_grad_kernel, grid, block, 0, S_(stream), dax, dah, db_x, db_h, (long)rows, N);
  return hip_status(hipGetLastError());
}

extern "C" int bmhrl_arelu_grad(const float* dy, const float* h, const float* alpha, const float* beta, float* partial,
                                float* dalpha, float* dbeta, int64_t n, bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG(dy && h && alpha && beta && partial && dalpha && dbeta && n > 0);
  hipLaunchKernelGGL(arelu_grad_partial_kernel, dim3(ARELU_PARTS), dim3(256), 0, S_(stream), dy, h, partial, (long)n);
  hipLaunchKernelGGL(arelu_grad_finish_kernel, dim3(1), dim3(64), 0, S_(stream), partial, alpha, beta, dalpha, dbeta);
  return hip_status(hipGetLastError());
}

extern "C" int bmhrl_critic_head_loss(const float* y2, const float* lin_w, const float* lin_b, const float* labels,
                                      const uint8_t* mask, float pos_weight, const float* ds_in, float* score, float* loss,
                                      float* ds, float* dy2, float* dlin_w, float* dlin_b, int64_t rows, int32_t H,
                                      bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG(y2 && lin_w && lin_b && ds && dy2 && dlin_w && dlin_b && rows > 0 && H > 0 && H <= MAXH && H % 4 == 0);
  BMHRL_CHECK_ARG(labels ? (mask != nullptr && loss != nullptr) : ds_in != nullptr);
  BMHRL_CHECK_ARG((((uintptr_t)y2 | (uintptr_t)lin_w | (uintptr_t)dy2) & 15) == 0);
  hipLaunchKernelGGL(critic_head_loss_kernel, dim3(1), dim3(1024), 0, S_(stream), y2, lin_w, lin_b, labels, mask, pos_weight,
                     ds_in, score, loss, ds, dy2, dlin_w, dlin_b, (long)rows, H);
  return hip_status(hipGetLastError());
}
