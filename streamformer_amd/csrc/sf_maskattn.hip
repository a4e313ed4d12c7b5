// Masked attention for training (streamformer_amd/masked_attention.py): the backward of sf_maskdec_attention_kernel and the mask packer.
// The forward is that kernel itself (sf_maskdec.hip, sf_op_maskattn_forward), which leaves stats[f, h, q] = log-sum-exp of the scaled
// scores over the visible keys (+inf for a query without one).  Nothing of the [F heads, Q, HW] probabilities is kept: both passes
// recompute P = exp(scale q.k - stats) on the visible keys, in fp32 with exact products (v_mfma_f32_16x16x4_f32), and
//     delta = rowsum(dO o ctx)      dV = P^T dO      dS = P o (dO V^T - delta)      dQ = scale dS K      dK = scale dS^T Q.
// delta is made by the MFMA tree that makes dP = dO V^T, with ctx rows in V's place: for a query with ONE visible key ctx = v, so
// dP - delta is exactly 0, as it is in softmax's own backward, and not the rounding of two differently ordered sums.
//
//   sf_maskattn_dq_kernel    the forward's shape: 256 threads = 4 waves on ONE 16-query tile of one (frame, head), key tiles dealt round-robin
//                            (tile t -> wave t % 4), q and dO of the lane's query in registers, K | V of a tile staged in the wave's own LDS
//                            area, S^T and dP^T by the forward's eight-chain tree, dQ^T += K^T dS^T.  The four partial dQ meet in LDS and are
//                            summed in wave order, then scaled.  LDS: 4 x 2 x 16 x (hd + 4) floats = 66 KB at head width 128.
//   sf_maskattn_dkv_kernel   256 threads = 4 waves, each OWNS one 16-key tile of one (frame, head) (64 consecutive keys per workgroup) with
//                            K and V of the lane's key in registers, and loops over the query tiles of that (frame, head): Q and dO of the
//                            16 queries, and their ctx, are staged once per workgroup (three [16][hd + 4] tiles and stats: 24.8 KB at width 128),
//                            S and dP by the same tree with the operands' roles swapped, dV^T += dO^T P, dK^T += Q^T dS.  Each key row has
//                            one owner and the query tiles come in ascending order: one summation order, no atomics.
//   SKIP: dq leaves out a key tile hidden from all 16 queries of its tile before K or V are loaded, exactly as the forward does.  dkv
//   leaves out a query tile before Q or dO are loaded when none of the workgroup's 64 keys is visible to any of its 16 queries (every
//   wave reads the 32 mask words that decide it, so the decision is uniform without a barrier), and a wave leaves out the arithmetic when
//   its own 16 keys are not.  Run unskipped (no_skip), such a pair has P = 0 and dS = 0 by selection, not by arithmetic, and an
//   accumulator that gets +-0 added keeps its bits (it is never -0: it starts at +0 and a cancelled sum rounds to +0).
//   Bits of keys at or past HW are never looked at: a key index is compared with HW before its bit is used, and the whole-word tests
//   mask the last word.
//   sf_maskattn_pack_kernel  bool [R, Q, HW] -> uint32 [R, Q, ceil(HW / 32)]: one wave per 64 keys of a row, one ballot, two words.
#include "sf_handle.h"

typedef __attribute__((ext_vector_type(4))) float ma4_t;

#define MKA_WAVES 4
#define MKA_MAX_HW (1 << 24)

struct SfMkaBwd {
  const float* q; const float* k; const float* v;      // fp32 rows; a head's columns at h * hd
  const uint32_t* mask;                                // [F, (heads,) Tq, words] or null
  const float* ctx; const float* stats; const float* d_ctx;      // [F Tq, heads * hd], [F, heads, Tq], [F Tq, heads * hd]
  float* dq; float* dk; float* dv;
  int q_pitch, kv_pitch, dq_pitch, dkv_pitch;
  int F, Tq, Tk, heads, hd, words, no_skip, mask_per_head;
  float scale;
};

SF_DEVICE ma4_t ma_mfma(float a, float b, ma4_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

SF_DEVICE const uint32_t* ma_mask_row(const SfMkaBwd& p, int f, int h, int q) {
  const size_t row = p.mask_per_head ? ((size_t)f * p.heads + h) * p.Tq + q : (size_t)f * p.Tq + q;
  return p.mask + row * p.words;
}

// the forward's score tree: rows (A operand, from LDS) x the lane's column (B operand, registers); eight chains
template <int NT>
SF_DEVICE ma4_t ma_scores(const float* rows, const float (&col)[NT * 4], int HDQ) {
  ma4_t part[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) part[j] = (ma4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < NT * 4; ++i)
    if (i < HDQ) part[i & 7] = ma_mfma(rows[4 * i], col[i], part[i & 7]);
  return ((part[0] + part[1]) + (part[2] + part[3])) + ((part[4] + part[5]) + (part[6] + part[7]));
}

// the same tree with both operands in LDS
template <int NT>
SF_DEVICE ma4_t ma_scores_lds(const float* rows, const float* col, int HDQ) {
  ma4_t part[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) part[j] = (ma4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < NT * 4; ++i)
    if (i < HDQ) part[i & 7] = ma_mfma(rows[4 * i], col[4 * i], part[i & 7]);
  return ((part[0] + part[1]) + (part[2] + part[3])) + ((part[4] + part[5]) + (part[6] + part[7]));
}

// ------------------------------------------------------------------------------------------------
// dQ
// ------------------------------------------------------------------------------------------------
template <int NT>
__global__ __launch_bounds__(64 * MKA_WAVES) void sf_maskattn_dq_kernel(SfMkaBwd p) {
  extern __shared__ __attribute__((aligned(16))) float ma_smem[];
  const int HD = p.hd, LD = HD + 4, HDQ = HD >> 2, Tq = p.Tq, Tk = p.Tk, C = p.heads * HD;
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63, l15 = lane & 15, g = lane >> 4;
  const int area = 2 * 16 * LD;
  float* kt = ma_smem + wave * area;
  float* vt = kt + 16 * LD;
  const int qtiles = (Tq + 15) >> 4;
  int b = (int)blockIdx.x;
  const int qt = b % qtiles; b /= qtiles;
  const int h = b % p.heads, f = b / p.heads;
  const int qi = qt * 16 + l15, qrow = qi < Tq ? qi : Tq - 1;      // lanes past Tq repeat the last query, see no key and store nothing
  for (int c = (int)threadIdx.x; c < 16 * HDQ; c += 64 * MKA_WAVES) {      // ctx of the 16 queries, for delta: the first wave's area
    const int row = c / HDQ, cc = c - row * HDQ, qo = qt * 16 + row < Tq ? qt * 16 + row : Tq - 1;
    *reinterpret_cast<ma4_t*>(ma_smem + row * LD + cc * 4) = *reinterpret_cast<const ma4_t*>(p.ctx + ((size_t)f * Tq + qo) * C + h * HD + cc * 4);
  }
  float qreg[NT * 4], doreg[NT * 4];
  {
    const float* q = p.q + ((size_t)f * Tq + qrow) * p.q_pitch + h * HD + g;      // k-index (g, i) of the score MFMAs is dim 4 i + g
    const float* dO = p.d_ctx + ((size_t)f * Tq + qrow) * C + h * HD + g;
#pragma unroll
    for (int i = 0; i < NT * 4; ++i) {
      qreg[i] = i < HDQ ? q[4 * i] : 0.f;
      doreg[i] = i < HDQ ? dO[4 * i] : 0.f;
    }
  }
  const float lse = p.stats[((size_t)f * p.heads + h) * Tq + qrow];
  const uint32_t* mrow = p.mask ? ma_mask_row(p, f, h, qrow) : nullptr;
  const size_t kv0 = (size_t)f * Tk;
  __syncthreads();
  // delta = dO . ctx by the tree that makes dP (ctx rows in V's place): a query with ONE visible key has ctx = v, so dP - delta is
  // exactly 0 there, as it is in softmax's own backward.  The tile is [query 4 g + r][query l15]; the diagonal is wanted.
  float delta;
  {
    const ma4_t dt = ma_scores<NT>(ma_smem + l15 * LD + g, doreg, HDQ);
    const int r = l15 & 3;
    const float mine = r == 0 ? dt[0] : r == 1 ? dt[1] : r == 2 ? dt[2] : dt[3];
    delta = __shfl(mine, (l15 >> 2) * 16 + l15, 64);
  }
  ma4_t acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = (ma4_t){0.f, 0.f, 0.f, 0.f};
  const int ntiles = (Tk + 15) >> 4, rounds = (ntiles + MKA_WAVES - 1) / MKA_WAVES;
  for (int r = 0; r < rounds; ++r) {                   // every wave runs every round: the barriers below are reached by all of them
    const int k0 = (r * MKA_WAVES + wave) * 16;
    bool active = k0 < Tk;
    unsigned vis = 0u, any = 0u;                       // bit j: key k0 + j is visible to this lane's query / to one of the 16 queries
    if (active) {
      const int nk = Tk - k0;
      const unsigned valid = nk >= 16 ? 0xffffu : ((1u << nk) - 1u);
      const unsigned hidden = mrow ? (mrow[k0 >> 5] >> (k0 & 31)) & 0xffffu : 0u;
      vis = qi < Tq ? (~hidden & valid) : 0u;
      any = vis;
      any |= __shfl_xor(any, 1, 64); any |= __shfl_xor(any, 2, 64); any |= __shfl_xor(any, 4, 64); any |= __shfl_xor(any, 8, 64);
      if (!p.no_skip && any == 0u) active = false;
    }
    __syncthreads();
    if (active) {
      for (int c = lane; c < 16 * HDQ; c += 64) {      // a key no query of the tile sees (and a row past Tk) is staged as zeros
        const int row = c / HDQ, cc = c - row * HDQ;
        ma4_t kv = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
        if ((any >> row) & 1u) {
          const size_t key = kv0 + k0 + row;
          kv = *reinterpret_cast<const ma4_t*>(p.k + key * p.kv_pitch + h * HD + cc * 4);
          vv = *reinterpret_cast<const ma4_t*>(p.v + key * p.kv_pitch + h * HD + cc * 4);
        }
        *reinterpret_cast<ma4_t*>(kt + row * LD + cc * 4) = kv;
        *reinterpret_cast<ma4_t*>(vt + row * LD + cc * 4) = vv;
      }
    }
    __syncthreads();
    if (active) {
      // S^T and dP^T tiles: keys k0 + l15 (A operand) x queries (B operand); lane (query l15, g) receives keys k0 + 4 g + r
      const ma4_t s4 = ma_scores<NT>(kt + l15 * LD + g, qreg, HDQ);
      const ma4_t dp4 = ma_scores<NT>(vt + l15 * LD + g, doreg, HDQ);
      float ds[4];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const bool ok = (vis >> (4 * g + rr)) & 1u;
        ds[rr] = ok ? expf(__fmul_rn(s4[rr], p.scale) - lse) * (dp4[rr] - delta) : 0.f;      // the forward's rounded product
      }
      // dQ^T += K^T dS^T: lane (dim l15 of the 16-dim tile, g) supplies K[k0 + 4 g + r][d]
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int d = t * 16 + l15;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const float kx = d < HD ? kt[(4 * g + rr) * LD + d] : 0.f;
          acc[t] = ma_mfma(kx, ds[rr], acc[t]);
        }
      }
    }
  }
  // ---- the four waves' partial results meet: each leaves dq [16][HD] in its own staging area ----
  __syncthreads();
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int d = t * 16 + 4 * g;
    if (d < HD) *reinterpret_cast<ma4_t*>(kt + l15 * HD + d) = acc[t];
  }
  __syncthreads();
  for (int idx = (int)threadIdx.x; idx < 16 * HDQ; idx += 64 * MKA_WAVES) {
    const int qq = idx / HDQ, d = (idx - qq * HDQ) * 4;
    const int qo = qt * 16 + qq;
    if (qo >= Tq) continue;
    ma4_t o = *reinterpret_cast<const ma4_t*>(ma_smem + qq * HD + d);
#pragma unroll
    for (int w = 1; w < MKA_WAVES; ++w) o += *reinterpret_cast<const ma4_t*>(ma_smem + w * area + qq * HD + d);      // wave order
    o *= p.scale;
    *reinterpret_cast<ma4_t*>(p.dq + ((size_t)f * Tq + qo) * p.dq_pitch + h * HD + d) = o;
  }
}

// ------------------------------------------------------------------------------------------------
// dK, dV
// ------------------------------------------------------------------------------------------------
template <int NT>
__global__ __launch_bounds__(64 * MKA_WAVES) void sf_maskattn_dkv_kernel(SfMkaBwd p) {
  extern __shared__ __attribute__((aligned(16))) float ma_smem[];
  const int HD = p.hd, LD = HD + 4, HDQ = HD >> 2, Tq = p.Tq, Tk = p.Tk, C = p.heads * HD;
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63, l15 = lane & 15, g = lane >> 4;
  float* qs = ma_smem;                                 // Q of the 16 queries [16][LD]
  float* dos = qs + 16 * LD;                           // dO [16][LD]
  float* cs = dos + 16 * LD;                           // ctx [16][LD]
  float* st = cs + 16 * LD;                            // stats [16]
  const int ntiles = (Tk + 15) >> 4, groups = (ntiles + MKA_WAVES - 1) / MKA_WAVES;
  int b = (int)blockIdx.x;
  const int kg = b % groups; b /= groups;
  const int h = b % p.heads, f = b / p.heads;
  const int kbase = kg * 16 * MKA_WAVES, k0 = kbase + wave * 16;
  const bool own = k0 < Tk;                            // a wave past the last key tile stages and waits with the others, nothing else
  const int ki = k0 + l15;
  const bool kvalid = ki < Tk;
  float kreg[NT * 4], vreg[NT * 4];
  {
    const size_t row = (size_t)f * Tk + (kvalid ? ki : Tk - 1);
    const float* k = p.k + row * p.kv_pitch + h * HD + g;      // B operand: lane (key l15, g) supplies dim 4 i + g
    const float* v = p.v + row * p.kv_pitch + h * HD + g;
#pragma unroll
    for (int i = 0; i < NT * 4; ++i) {
      kreg[i] = i < HDQ ? k[4 * i] : 0.f;
      vreg[i] = i < HDQ ? v[4 * i] : 0.f;
    }
  }
  ma4_t dk_acc[NT], dv_acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) { dk_acc[t] = (ma4_t){0.f, 0.f, 0.f, 0.f}; dv_acc[t] = (ma4_t){0.f, 0.f, 0.f, 0.f}; }
  const int qtiles = (Tq + 15) >> 4;
  for (int qt = 0; qt < qtiles; ++qt) {
    const int q0 = qt * 16;
    // ---- is any of the workgroup's 64 keys visible to any of the 16 queries?  32 words, the same in every wave ----
    if (!p.no_skip && p.mask) {
      unsigned v = 0u;
      const int qo = q0 + l15, w = (kbase >> 5) + (g & 1);
      if (lane < 32 && qo < Tq && w < p.words) {
        const int nk = Tk - w * 32;
        v = ~ma_mask_row(p, f, h, qo)[w] & (nk >= 32 ? 0xffffffffu : ((1u << nk) - 1u));
      }
      if (__ballot(v != 0u) == 0ull) continue;          // uniform over the workgroup: no barrier is passed by a part of it
    }
    // ---- which of the lane's four (query q0 + 4 g + r, key ki) pairs are visible ----
    unsigned vis = 0u;
    if (own && kvalid) {
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int qo = q0 + 4 * g + rr;
        if (qo < Tq && !(p.mask && ((ma_mask_row(p, f, h, qo)[ki >> 5] >> (ki & 31)) & 1u))) vis |= 1u << rr;
      }
    }
    const bool wave_act = p.no_skip ? own : __ballot(vis != 0u) != 0ull;
    __syncthreads();                                   // the previous query tile has been read
    for (int c = (int)threadIdx.x; c < 16 * HDQ; c += 64 * MKA_WAVES) {
      const int row = c / HDQ, cc = c - row * HDQ;
      ma4_t qv = {0.f, 0.f, 0.f, 0.f}, dv = {0.f, 0.f, 0.f, 0.f}, cv = {0.f, 0.f, 0.f, 0.f};
      if (q0 + row < Tq) {
        qv = *reinterpret_cast<const ma4_t*>(p.q + ((size_t)f * Tq + q0 + row) * p.q_pitch + h * HD + cc * 4);
        dv = *reinterpret_cast<const ma4_t*>(p.d_ctx + ((size_t)f * Tq + q0 + row) * C + h * HD + cc * 4);
        cv = *reinterpret_cast<const ma4_t*>(p.ctx + ((size_t)f * Tq + q0 + row) * C + h * HD + cc * 4);
      }
      *reinterpret_cast<ma4_t*>(qs + row * LD + cc * 4) = qv;
      *reinterpret_cast<ma4_t*>(dos + row * LD + cc * 4) = dv;
      *reinterpret_cast<ma4_t*>(cs + row * LD + cc * 4) = cv;
    }
    if (threadIdx.x < 16) st[threadIdx.x] = q0 + (int)threadIdx.x < Tq ? p.stats[((size_t)f * p.heads + h) * Tq + q0 + threadIdx.x] : INFINITY;
    __syncthreads();
    if (wave_act) {
      // S and dP tiles: queries q0 + l15 (A operand, LDS) x keys (B operand, registers); lane (key l15, g) receives queries q0 + 4 g + r
      const ma4_t s4 = ma_scores<NT>(qs + l15 * LD + g, kreg, HDQ);
      const ma4_t dp4 = ma_scores<NT>(dos + l15 * LD + g, vreg, HDQ);
      // delta as in the dq pass, by dP's tree with ctx rows in V's place: [query 4 g + r][query l15], the diagonal to the lanes that want it
      const ma4_t dt = ma_scores_lds<NT>(dos + l15 * LD + g, cs + l15 * LD + g, HDQ);
      float pr[4], ds[4];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const bool ok = (vis >> rr) & 1u;
        const float delta = __shfl(dt[rr], 20 * g + rr, 64);      // lane (query 4 g + r, g) holds it in element r
        pr[rr] = ok ? expf(__fmul_rn(s4[rr], p.scale) - st[4 * g + rr]) : 0.f;
        ds[rr] = ok ? pr[rr] * (dp4[rr] - delta) : 0.f;
      }
      // dV^T += dO^T P, dK^T += Q^T dS: lane (dim l15 of the 16-dim tile, g) supplies dO | Q [q0 + 4 g + r][d]
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int d = t * 16 + l15;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const float dx = d < HD ? dos[(4 * g + rr) * LD + d] : 0.f;
          const float qx = d < HD ? qs[(4 * g + rr) * LD + d] : 0.f;
          dv_acc[t] = ma_mfma(dx, pr[rr], dv_acc[t]);
          dk_acc[t] = ma_mfma(qx, ds[rr], dk_acc[t]);
        }
      }
    }
  }
  if (own && kvalid) {                                 // lane (key l15, g) holds dims 16 t + 4 g .. + 3 of its key
    const size_t ob = ((size_t)f * Tk + ki) * p.dkv_pitch + h * HD;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int d = t * 16 + 4 * g;
      if (d < HD) {
        *reinterpret_cast<ma4_t*>(p.dk + ob + d) = dk_acc[t] * p.scale;
        *reinterpret_cast<ma4_t*>(p.dv + ob + d) = dv_acc[t];
      }
    }
  }
}

static hipError_t mka_launch_backward(const SfMkaBwd& p, hipStream_t s) {
  const int64_t dq_blocks = (int64_t)p.F * p.heads * ((p.Tq + 15) / 16);
  const int64_t dkv_blocks = (int64_t)p.F * p.heads * (((p.Tk + 15) / 16 + MKA_WAVES - 1) / MKA_WAVES);
  if (dq_blocks > 0x7fffffff || dkv_blocks > 0x7fffffff) return hipErrorInvalidValue;
  const size_t dq_lds = (size_t)MKA_WAVES * 2 * 16 * (p.hd + 4) * sizeof(float);      // 66 KB at head_dim 128
  const size_t dkv_lds = ((size_t)3 * 16 * (p.hd + 4) + 16) * sizeof(float);          // 24.8 KB
  const dim3 block(64 * MKA_WAVES);
  hipError_t e;
  switch ((p.hd + 15) / 16) {
#define MA_CASE(E)                                                                                              \
  case E:                                                                                                       \
    e = sf_launch_big_lds(sf_maskattn_dq_kernel<E>, dim3((unsigned)dq_blocks), block, dq_lds, s, p);            \
    if (e != hipSuccess) return e;                                                                              \
    return sf_launch(sf_maskattn_dkv_kernel<E>, dim3((unsigned)dkv_blocks), block, dkv_lds, s, p);
    MA_CASE(1) MA_CASE(2) MA_CASE(3) MA_CASE(4) MA_CASE(5) MA_CASE(6) MA_CASE(7) MA_CASE(8)
#undef MA_CASE
    default: return hipErrorInvalidValue;
  }
}

extern "C" int sf_op_maskattn_backward(const float* q_dev, int q_pitch, const float* k_dev, const float* v_dev, int kv_pitch, const uint32_t* mask_dev,
                                       int mask_per_head, const float* ctx_dev, const float* stats_dev, const float* d_ctx_dev, float* dq_dev,
                                       int dq_pitch, float* dk_dev, float* dv_dev, int dkv_pitch, int F, int Q, int HW, int heads, int head_dim,
                                       int no_skip, sf_stream stream) {
  const char* who = "sf_op_maskattn_backward";
  if (!q_dev || !k_dev || !v_dev || !ctx_dev || !stats_dev || !d_ctx_dev || !dq_dev || !dk_dev || !dv_dev) return sf_set_err(SF_ERR_INVALID, "%s: null buffer", who);
  if (F < 1 || F > 65535 || Q < 1 || Q > 65535 || HW < 1 || HW > MKA_MAX_HW || heads < 1 || heads > 65535)
    return sf_set_err(SF_ERR_INVALID, "%s: bad shape F=%d (1..65535) Q=%d (1..65535) HW=%d (1..%d) heads=%d", who, F, Q, HW, MKA_MAX_HW, heads);
  if (head_dim < 8 || head_dim > 128 || head_dim % 8) return sf_set_err(SF_ERR_INVALID, "%s: head_dim must be a multiple of 8 in 8..128", who);
  const int D = heads * head_dim;
  if (q_pitch < D || kv_pitch < D || dq_pitch < D || dkv_pitch < D || ((q_pitch | kv_pitch | dq_pitch | dkv_pitch) & 3))
    return sf_set_err(SF_ERR_INVALID, "%s: row pitches must be multiples of 4 and at least heads * head_dim = %d", who, D);
  if ((int64_t)F * (Q > HW ? Q : HW) * std::max(std::max(q_pitch, kv_pitch), std::max(dq_pitch, dkv_pitch)) > (int64_t)0x7fffffff)
    return sf_set_err(SF_ERR_CAPACITY, "%s: more than 2^31 - 1 elements", who);
  if (((uintptr_t)q_dev | (uintptr_t)k_dev | (uintptr_t)v_dev | (uintptr_t)mask_dev | (uintptr_t)ctx_dev | (uintptr_t)stats_dev | (uintptr_t)d_ctx_dev |
       (uintptr_t)dq_dev | (uintptr_t)dk_dev | (uintptr_t)dv_dev) & 15)
    return sf_set_err(SF_ERR_INVALID, "%s: buffers must be 16-byte aligned", who);
  SfMkaBwd a;
  memset(&a, 0, sizeof(a));
  a.q = q_dev; a.k = k_dev; a.v = v_dev; a.mask = mask_dev; a.ctx = ctx_dev; a.stats = stats_dev; a.d_ctx = d_ctx_dev;
  a.dq = dq_dev; a.dk = dk_dev; a.dv = dv_dev;
  a.q_pitch = q_pitch; a.kv_pitch = kv_pitch; a.dq_pitch = dq_pitch; a.dkv_pitch = dkv_pitch;
  a.F = F; a.Tq = Q; a.Tk = HW; a.heads = heads; a.hd = head_dim; a.words = (HW + 31) / 32; a.no_skip = no_skip ? 1 : 0;
  a.mask_per_head = mask_dev && mask_per_head ? 1 : 0;
  a.scale = 1.0f / sqrtf((float)head_dim);
  HIP_TRY(mka_launch_backward(a, (hipStream_t)stream));
  return SF_OK;
}

// ------------------------------------------------------------------------------------------------
// bool mask -> packed words
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sf_maskattn_pack_kernel(const uint8_t* in, uint32_t* out, long long rows, int HW, int words) {
  const int lane = (int)threadIdx.x & 63, chunks = (HW + 63) >> 6;
  const long long units = rows * chunks, step = (long long)gridDim.x * (blockDim.x >> 6);
  for (long long u = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); u < units; u += step) {
    const long long row = u / chunks;
    const int ch = (int)(u - row * chunks), key = ch * 64 + lane;
    const bool hidden = key >= HW || in[row * HW + key] != 0;      // padding bits are set
    const unsigned long long bits = __ballot(hidden);
    if (lane < 2 && 2 * ch + lane < words) out[row * words + 2 * ch + lane] = (uint32_t)(bits >> (32 * lane));
  }
}

extern "C" int sf_op_maskattn_pack(const uint8_t* mask_dev, uint32_t* bits_dev, long long rows, int HW, sf_stream stream) {
  const char* who = "sf_op_maskattn_pack";
  if (!mask_dev || !bits_dev) return sf_set_err(SF_ERR_INVALID, "%s: null buffer", who);
  if (rows < 1 || HW < 1 || HW > MKA_MAX_HW) return sf_set_err(SF_ERR_INVALID, "%s: bad shape rows=%lld HW=%d (1..%d)", who, rows, HW, MKA_MAX_HW);
  if ((uintptr_t)bits_dev & 3) return sf_set_err(SF_ERR_INVALID, "%s: bits_dev must be 4-byte aligned", who);
  const int words = (HW + 31) / 32;
  if (rows > 0x7fffffffLL * 32 / HW) return sf_set_err(SF_ERR_CAPACITY, "%s: more than 2^36 mask elements", who);
  const long long units = rows * ((HW + 63) / 64);
  const long long grid = std::min<long long>((units + 3) / 4, 65536);
  HIP_TRY(sf_launch(sf_maskattn_pack_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, mask_dev, bits_dev, rows, HW, words));
  return SF_OK;
}
