// CTVIS contrastive loss: the device side of CTCLPlugin (ctvis/modeling/cl_plugin/ct_cl_plugin.py).  All fp32, on the caller's stream,
// without allocation or host synchronisation; the launch count does not depend on the videos, frames, instances or items; no float
// atomics and every sum in a fixed order, so two runs give the same bits.
//
// The host decides the data-dependent bookkeeping (streamformer_amd/cl_plugin.py, Plan) and uploads it as int32 tables:
//   track_rows [T, F]   the matched row (b F + f) Q + q of a (video, instance) at every frame it is present in, else -1
//   track_items [T, F]  the item whose anchor is (track, frame), or -1
//   items [I, 8]        track, frame, anchor row, positive kind (0: embedding row, 1: sg row t F + f'), positive index, first negative,
//                       negatives, positive frame
//   neg [NE]            the items' negative rows; row_start [R + 1], row_items [NE]: per row the items that list it, in plan order
// A row of C floats (C a multiple of 8 up to 256) is held by one wave, four channels a lane, one 16-byte load.
//
//   sf_clp_tracks_kernel      one workgroup per track: the present embeddings and their inverse norms in LDS, every pair's cosine by a wave,
//                             sim and beta = max(0, sim) per present frame, then the recurrence sg = (1 - beta) sg + beta e along the frames,
//                             a thread a channel; absent frames repeat the value before.
//   sf_clp_items_kernel       one workgroup per item: the anchor in registers, the 1 + n rows over the four waves (dot and norm by wave
//                             reduction), then wave 0: log(1 + sum exp(d_neg - d_pos)) with the maximum subtracted, and the aux mean.
//   sf_clp_finish_kernel      the two sums in item order, over the item count.
//   sf_clp_item_bwd_kernel    one workgroup per item: the gradient of its anchor and of its positive, into the workspace.
//   sf_clp_neg_bwd_kernel     one wave per row of grad_pred_embeds: a gather over the items that list the row as a negative; rows nobody
//                             lists are written as zeros.
//   sf_clp_track_bwd_kernel   one workgroup per track owns its matched rows (a bijection per frame: owners never collide): adds the anchor
//                             and positive terms, runs the recurrence backwards (with d beta where sim > 0) and adds the result to the rows.
#include "sf_internal.h"
#include "sf_common.h"
#include "sf_launch.h"
#include "sf_handle.h"

#define CLP_MAX_C 256
#define CLP_MAX_F 32                       // frames of a track: three [F][C] planes of the backward stay in LDS
#define CLP_MAX_NEG 4096                   // negatives of an item
#define CLP_EPS 1e-12f                     // F.normalize's eps

SF_DEVICE float clp_dot(const float4& a, const float4& b) { return (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w); }
SF_DEVICE float4 clp_row(const float* base, size_t row, int C, int lane) {
  return lane * 4 < C ? *reinterpret_cast<const float4*>(base + row * (size_t)C + lane * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
}
SF_DEVICE int clp_clamp(int v, int n) { return (unsigned)v < (unsigned)n ? v : 0; }      // a table entry out of range reads row 0, never outside

// ------------------------------------------------------------------------------------------------
// tracks: similarity-guided embeddings
// ------------------------------------------------------------------------------------------------
struct ClpTrackArgs {
  const float* emb; const float* sg_in; const float* stats_in; const int32_t* track_rows; const int32_t* track_items; const int32_t* items;
  const float* ga; const float* gp;        // backward: per item the gradient of the anchor and of the positive [I, C]
  float* sg; float* stats; float* grad;
  int R, C, F, I;
};

// the prologue both track kernels share: present frames fr[0..m), their embeddings E[j][C], inverse norms and the pairs' cosines
SF_DEVICE int clp_track_load(const ClpTrackArgs& p, int t, float* E, float* cosm, float* inv, int* fr, int* m_s) {
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int32_t* rows = p.track_rows + (size_t)t * p.F;
  if (tid == 0) {
    int m = 0;
    for (int f = 0; f < p.F; ++f)
      if ((unsigned)rows[f] < (unsigned)p.R) fr[m++] = f;
    *m_s = m;
  }
  __syncthreads();
  const int m = *m_s;
  for (int j = wave; j < m; j += 4) {
    const float4 v = clp_row(p.emb, (size_t)rows[fr[j]], p.C, lane);
    if (lane * 4 < p.C) *reinterpret_cast<float4*>(E + j * p.C + lane * 4) = v;
    const float s = wave_sum(clp_dot(v, v));
    if (lane == 0) inv[j] = 1.f / fmaxf(sqrtf(s), CLP_EPS);
  }
  __syncthreads();
  for (int pr = wave; pr < m * m; pr += 4) {
    const int j = pr / m, i = pr - j * m;
    if (i >= j) continue;                                      // the whole wave
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    if (lane * 4 < p.C) {
      a = *reinterpret_cast<const float4*>(E + i * p.C + lane * 4);
      b = *reinterpret_cast<const float4*>(E + j * p.C + lane * 4);
    }
    const float ii = inv[i], ij = inv[j];
    a.x *= ii; a.y *= ii; a.z *= ii; a.w *= ii;
    b.x *= ij; b.y *= ij; b.z *= ij; b.w *= ij;
    const float c = wave_sum(clp_dot(a, b));
    if (lane == 0) cosm[j * p.F + i] = c;
  }
  __syncthreads();
  return m;
}

__global__ __launch_bounds__(256) void sf_clp_tracks_kernel(ClpTrackArgs p) {
  extern __shared__ __attribute__((aligned(16))) float clp_smem[];
  float* E = clp_smem;                                        // [F][C]
  float* cosm = E + p.F * p.C;                                // [F][F]
  float* inv = cosm + p.F * p.F;                              // [F]
  float* beta = inv + p.F;                                    // [F]
  float* simv = beta + p.F;                                   // [F]
  int* fr = reinterpret_cast<int*>(simv + p.F);               // [F]
  int* m_s = fr + p.F;                                        // dynamic as well: the launch helper gives the dynamic part the CU's whole LDS
  const int tid = (int)threadIdx.x, t = (int)blockIdx.x;
  const int m = clp_track_load(p, t, E, cosm, inv, fr, m_s);
  if (tid == 0) {
    if (m > 0) { simv[0] = 0.f; beta[0] = 0.f; }
    for (int j = 1; j < m; ++j) {
      float s = 0.f;
      for (int i = 0; i < j; ++i) s += cosm[j * p.F + i];
      const float sim = s / (float)j;
      simv[j] = sim;
      beta[j] = sim > 0.f ? sim : 0.f;                         // max(0, sim)
    }
  }
  __syncthreads();
  if (tid < p.C) {
    float sg = 0.f;
    int j = -1;
    for (int f = 0; f < p.F; ++f) {
      if (j + 1 < m && fr[j + 1] == f) {
        ++j;
        const float e = E[j * p.C + tid];
        sg = j == 0 ? e : (1.f - beta[j]) * sg + beta[j] * e;
      }
      p.sg[((size_t)t * p.F + f) * p.C + tid] = sg;            // before the first present frame: zeros
    }
  }
  if (tid < p.F) {
    float s = 0.f, b = 0.f;
    for (int j = 0; j < m; ++j)
      if (fr[j] == tid) { s = simv[j]; b = beta[j]; }
    p.stats[((size_t)t * p.F + tid) * 2] = s;
    p.stats[((size_t)t * p.F + tid) * 2 + 1] = b;
  }
}

// ------------------------------------------------------------------------------------------------
// items: the per-item losses
// ------------------------------------------------------------------------------------------------
struct ClpItemArgs {
  const float* emb; const float* sg; const int32_t* items; const int32_t* neg; const int32_t* row_start; const int32_t* row_items;
  const float* up;                         // backward: d / d (loss_reid, loss_aux_reid)
  float* item_out;                         // [I, 4]: contras, aux, d_pos, 1 / |anchor|
  float* ga; float* gp; float* grad;
  int R, C, T, F, I, NE, ld;               // ld: 1 + the largest negative count
};
struct ClpItem { int a_row, kind, pos, n0, n; };

SF_DEVICE ClpItem clp_item(const ClpItemArgs& p, int item) {
  const int32_t* it = p.items + 8 * (size_t)item;
  ClpItem r;
  r.a_row = clp_clamp(it[2], p.R);
  r.kind = it[3] != 0;
  r.pos = clp_clamp(it[4], r.kind ? p.T * p.F : p.R);
  r.n = min(max(it[6], 0), p.ld - 1);
  r.n0 = min(max(it[5], 0), max(p.NE - r.n, 0));
  r.n = min(r.n, p.NE - r.n0);
  return r;
}
SF_DEVICE float4 clp_item_row(const ClpItemArgs& p, const ClpItem& it, int j, int lane) {      // row 0 is the positive
  if (j == 0) return clp_row(it.kind ? p.sg : p.emb, (size_t)it.pos, p.C, lane);
  return clp_row(p.emb, (size_t)clp_clamp(p.neg[it.n0 + j - 1], p.R), p.C, lane);
}

__global__ __launch_bounds__(256) void sf_clp_items_kernel(ClpItemArgs p) {
  extern __shared__ __attribute__((aligned(16))) float clp_smem[];
  float* d = clp_smem;                                        // [ld]
  float* cs = d + p.ld;                                       // [ld]
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, item = (int)blockIdx.x;
  const ClpItem it = clp_item(p, item);
  const float4 a = clp_row(p.emb, (size_t)it.a_row, p.C, lane);
  const float inv_a = 1.f / fmaxf(sqrtf(wave_sum(clp_dot(a, a))), CLP_EPS);
  for (int j = wave; j <= it.n; j += 4) {
    const float4 v = clp_item_row(p, it, j, lane);
    const float dj = wave_sum(clp_dot(v, a)), nr = sqrtf(wave_sum(clp_dot(v, v)));
    if (lane == 0) { d[j] = dj; cs[j] = dj * (1.f / fmaxf(nr, CLP_EPS)) * inv_a; }
  }
  __syncthreads();
  if (wave != 0) return;
  const float dpos = d[0];
  float mx = 0.f;                                             // the appended 0 of the reference's logsumexp
  for (int k = 1 + lane; k <= it.n; k += 64) mx = fmaxf(mx, d[k] - dpos);
  mx = wave_max(mx);
  float s = 0.f, ax = 0.f;
  for (int k = 1 + lane; k <= it.n; k += 64) {
    s += expf((d[k] - dpos) - mx);
    ax += cs[k] * cs[k];
  }
  s = wave_sum_dpp(s);
  ax = wave_sum_dpp(ax);
  if (lane == 0) {
    float* o = p.item_out + 4 * (size_t)item;
    o[0] = mx == 0.f ? log1pf(s) : mx + logf(expf(-mx) + s);
    o[1] = ((cs[0] - 1.f) * (cs[0] - 1.f) + ax) / (float)(it.n + 1);
    o[2] = dpos;
    o[3] = inv_a;
  }
}

__global__ __launch_bounds__(64) void sf_clp_finish_kernel(const float* item_out, int I, float* losses) {
  const int v = (int)threadIdx.x;
  if (v >= 2) return;
  float a = 0.f;
  for (int n = 0; n < I; ++n) a += item_out[4 * (size_t)n + v];                 // item order
  losses[v] = I > 0 ? a / (float)I : 0.f;
}

// ------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------
// d loss / d cos of a row, times 2 / (I (1 + n)); d loss / d dot of a negative is up0 / I times its softmax weight exp(d - d_pos - contras)
__global__ __launch_bounds__(256) void sf_clp_item_bwd_kernel(ClpItemArgs p) {
  __shared__ __attribute__((aligned(16))) float part[4][CLP_MAX_C];
  __shared__ float gam[4];
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, item = (int)blockIdx.x;
  const ClpItem it = clp_item(p, item);
  const float* o = p.item_out + 4 * (size_t)item;
  const float L = o[0], dpos = o[2], inv_a = o[3];
  const bool nz_a = inv_a < 1.f / CLP_EPS;
  const float u0 = p.up[0] / (float)p.I, u1 = 2.f * p.up[1] / ((float)p.I * (float)(it.n + 1));
  const float W = -expm1f(-L);                                // the sum of the negatives' softmax weights
  const float4 a = clp_row(p.emb, (size_t)it.a_row, p.C, lane);
  float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
  float gm = 0.f;
  for (int j = wave; j <= it.n; j += 4) {
    const float4 v = clp_item_row(p, it, j, lane);
    const float dj = wave_sum(clp_dot(v, a)), nr = sqrtf(wave_sum(clp_dot(v, v)));
    const float inv_r = 1.f / fmaxf(nr, CLP_EPS);
    const float c = dj * inv_r * inv_a;
    const float ec = u1 * (c - (j == 0 ? 1.f : 0.f));
    const float wd = j == 0 ? -u0 * W : u0 * expf((dj - dpos) - L);
    const float alpha = wd + ec * inv_r * inv_a;
    g.x += alpha * v.x; g.y += alpha * v.y; g.z += alpha * v.z; g.w += alpha * v.w;
    if (nz_a) gm -= ec * c * inv_a * inv_a;
    if (j == 0 && lane * 4 < p.C) {                            // the positive's own gradient
      const float back = nr > CLP_EPS ? ec * c * inv_r * inv_r : 0.f;
      *reinterpret_cast<float4*>(p.gp + (size_t)item * p.C + lane * 4) =
          make_float4(alpha * a.x - back * v.x, alpha * a.y - back * v.y, alpha * a.z - back * v.z, alpha * a.w - back * v.w);
    }
  }
  if (lane * 4 < p.C) *reinterpret_cast<float4*>(&part[wave][lane * 4]) = g;
  if (lane == 0) gam[wave] = gm;
  __syncthreads();
  if (tid < p.C) {
    const float ac = p.emb[(size_t)it.a_row * p.C + tid];
    p.ga[(size_t)item * p.C + tid] = ((part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid])) + ((gam[0] + gam[1]) + (gam[2] + gam[3])) * ac;
  }
}

__global__ __launch_bounds__(256) void sf_clp_neg_bwd_kernel(ClpItemArgs p) {
  const int lane = (int)threadIdx.x & 63, row = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (row >= p.R) return;
  const int s0 = min(max(p.row_start[row], 0), p.NE), s1 = min(max(p.row_start[row + 1], s0), p.NE);
  float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
  if (s1 > s0) {
    const float4 v = clp_row(p.emb, (size_t)row, p.C, lane);
    const float nr = sqrtf(wave_sum(clp_dot(v, v))), inv_r = 1.f / fmaxf(nr, CLP_EPS);
    const float u0 = p.up[0] / (float)p.I;
    for (int e = s0; e < s1; ++e) {                            // plan order
      const int item = clp_clamp(p.row_items[e], p.I);
      const ClpItem it = clp_item(p, item);
      const float* o = p.item_out + 4 * (size_t)item;
      const float L = o[0], dpos = o[2], inv_a = o[3];
      const float4 a = clp_row(p.emb, (size_t)it.a_row, p.C, lane);
      const float dj = wave_sum(clp_dot(v, a));
      const float c = dj * inv_r * inv_a;
      const float ec = 2.f * p.up[1] / ((float)p.I * (float)(it.n + 1)) * c;
      const float alpha = u0 * expf((dj - dpos) - L) + ec * inv_r * inv_a;
      const float back = nr > CLP_EPS ? ec * c * inv_r * inv_r : 0.f;
      g.x += alpha * a.x - back * v.x; g.y += alpha * a.y - back * v.y; g.z += alpha * a.z - back * v.z; g.w += alpha * a.w - back * v.w;
    }
  }
  if (lane * 4 < p.C) *reinterpret_cast<float4*>(p.grad + (size_t)row * p.C + lane * 4) = g;
}

__global__ __launch_bounds__(256) void sf_clp_track_bwd_kernel(ClpTrackArgs p) {
  extern __shared__ __attribute__((aligned(16))) float clp_smem[];
  float* E = clp_smem;                                        // [F][C]
  float* gE = E + p.F * p.C;                                  // [F][C]: d / d e_j
  float* gS = gE + p.F * p.C;                                 // [F][C]: d / d sg_j, then the scanned value
  float* cosm = gS + p.F * p.C;                               // [F][F]
  float* inv = cosm + p.F * p.F;                              // [F]
  float* beta = inv + p.F;                                    // [F]
  float* dbeta = beta + p.F;                                  // [F]
  int* fr = reinterpret_cast<int*>(dbeta + p.F);              // [F]: frame of present index j
  int* last = fr + p.F;                                       // [F]: the last present index at or before frame f, or -1
  int* m_s = last + p.F;
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, t = (int)blockIdx.x;
  const int m = clp_track_load(p, t, E, cosm, inv, fr, m_s);
  if (m == 0) return;
  if (tid == 0) {
    int j = -1;
    for (int f = 0; f < p.F; ++f) {
      if (j + 1 < m && fr[j + 1] == f) ++j;
      last[f] = j;
    }
    for (int k = 0; k < m; ++k) { beta[k] = p.stats_in[((size_t)t * p.F + fr[k]) * 2 + 1]; dbeta[k] = 0.f; }
  }
  __syncthreads();
  const int32_t* rows = p.track_rows + (size_t)t * p.F;
  const bool own = tid < p.C;
  if (own) {
    for (int j = 0; j < m; ++j) { gE[j * p.C + tid] = 0.f; gS[j * p.C + tid] = 0.f; }
    for (int f = 1; f < p.F; ++f) {                            // the track's items in frame order
      const int item = p.track_items[(size_t)t * p.F + f];
      if ((unsigned)item >= (unsigned)p.I || last[f] < 0) continue;
      const int32_t* it = p.items + 8 * (size_t)item;
      const int kind = it[3] != 0, jp = last[clp_clamp(it[7], p.F)];
      gE[last[f] * p.C + tid] += p.ga[(size_t)item * p.C + tid];
      if (jp >= 0) (kind ? gS : gE)[jp * p.C + tid] += p.gp[(size_t)item * p.C + tid];
    }
    float carry = 0.f;                                         // the recurrence backwards: sg_j = (1 - beta_j) sg_{j-1} + beta_j e_j
    for (int j = m - 1; j >= 1; --j) {
      const float gs = gS[j * p.C + tid] + carry;
      gS[j * p.C + tid] = gs;
      gE[j * p.C + tid] += beta[j] * gs;
      carry = (1.f - beta[j]) * gs;
    }
    gE[tid] += gS[tid] + carry;
  }
  __syncthreads();
  for (int j = 1 + wave; j < m; j += 4) {                      // d beta_j = gs_j . (e_j - sg_{j-1}), where sim_j > 0
    float4 gs = make_float4(0.f, 0.f, 0.f, 0.f), df = gs;
    if (lane * 4 < p.C) {
      gs = *reinterpret_cast<const float4*>(gS + j * p.C + lane * 4);
      const float4 e = *reinterpret_cast<const float4*>(E + j * p.C + lane * 4);
      const float4 s = *reinterpret_cast<const float4*>(p.sg_in + ((size_t)t * p.F + fr[j - 1]) * p.C + lane * 4);
      df = make_float4(e.x - s.x, e.y - s.y, e.z - s.z, e.w - s.w);
    }
    const float db = wave_sum(clp_dot(gs, df));
    if (lane == 0) dbeta[j] = beta[j] > 0.f ? db : 0.f;
  }
  __syncthreads();
  if (!own) return;
  for (int j = 1; j < m; ++j) {                                // sim_j = sum_i cos(e_i, e_j) / j
    if (dbeta[j] == 0.f) continue;
    const float dc = dbeta[j] / (float)j, hj = E[j * p.C + tid] * inv[j];
    const bool nz_j = inv[j] < 1.f / CLP_EPS;
    float gj = 0.f;
    for (int i = 0; i < j; ++i) {
      const float c = cosm[j * p.F + i], hi = E[i * p.C + tid] * inv[i];
      const bool nz_i = inv[i] < 1.f / CLP_EPS;
      gE[i * p.C + tid] += dc * (hj - (nz_i ? c * hi : 0.f)) * inv[i];
      gj += dc * (hi - (nz_j ? c * hj : 0.f)) * inv[j];
    }
    gE[j * p.C + tid] += gj;
  }
  for (int j = 0; j < m; ++j) p.grad[(size_t)rows[fr[j]] * p.C + tid] += gE[j * p.C + tid];
}

// ------------------------------------------------------------------------------------------------
// entry points: every refusal happens before anything is launched
// ------------------------------------------------------------------------------------------------
static size_t clp_align(size_t b) { return (b + 255) & ~(size_t)255; }

static int clp_shape(const char* who, int R, int C, int T, int F) {
  if (R < 1 || T < 0 || F < 1) return sf_set_err(SF_ERR_INVALID, "%s: R = %d rows, T = %d tracks, F = %d frames", who, R, T, F);
  if (C < 8 || C > CLP_MAX_C || C % 8) return sf_set_err(SF_ERR_CAPACITY, "%s: C = %d channels: a multiple of 8 up to %d", who, C, CLP_MAX_C);
  if (F > CLP_MAX_F) return sf_set_err(SF_ERR_CAPACITY, "%s: F = %d frames exceed %d (a track's frames stay in the CU's LDS)", who, F, CLP_MAX_F);
  if ((long long)T * F > 0x7fffffffLL / CLP_MAX_C) return sf_set_err(SF_ERR_CAPACITY, "%s: T F = %lld exceeds the index range", who, (long long)T * F);
  return SF_OK;
}
static int clp_items_shape(const char* who, int I, int NE, int max_neg) {
  if (I < 0 || NE < 0 || max_neg < 0) return sf_set_err(SF_ERR_INVALID, "%s: I = %d items, NE = %d negative rows, max_neg = %d", who, I, NE, max_neg);
  if (max_neg > CLP_MAX_NEG) return sf_set_err(SF_ERR_CAPACITY, "%s: %d negatives of an item exceed %d", who, max_neg, CLP_MAX_NEG);
  return SF_OK;
}

extern "C" int sf_op_clp_tracks(const float* embeds_dev, int R, int C, const int32_t* track_rows_dev, int T, int F, float* sg_dev, float* stats_dev,
                                sf_stream stream) {
  const char* who = "sf_op_clp_tracks";
  if (!embeds_dev || !sg_dev || !stats_dev || (T > 0 && !track_rows_dev)) return sf_set_err(SF_ERR_INVALID, "%s: null buffer", who);
  SF_TRY(clp_shape(who, R, C, T, F));
  if (T == 0) return SF_OK;
  ClpTrackArgs p = {};
  p.emb = embeds_dev; p.track_rows = track_rows_dev; p.sg = sg_dev; p.stats = stats_dev; p.R = R; p.C = C; p.F = F;
  const size_t lds = ((size_t)F * C + (size_t)F * F + 4 * (size_t)F + 4) * 4;
  HIP_TRY(sf_launch_big_lds(sf_clp_tracks_kernel, dim3((unsigned)T), dim3(256), lds, (hipStream_t)stream, p));
  return SF_OK;
}

extern "C" int sf_op_clp_items(const float* embeds_dev, int R, int C, const float* sg_dev, int T, int F, const int32_t* items_dev, int I,
                               const int32_t* neg_dev, int NE, int max_neg, float* losses_dev, float* item_out_dev, sf_stream stream) {
  const char* who = "sf_op_clp_items";
  if (!embeds_dev || !sg_dev || !losses_dev || (I > 0 && (!items_dev || !item_out_dev)) || (NE > 0 && !neg_dev))
    return sf_set_err(SF_ERR_INVALID, "%s: null buffer", who);
  SF_TRY(clp_shape(who, R, C, T, F));
  SF_TRY(clp_items_shape(who, I, NE, max_neg));
  ClpItemArgs p = {};
  p.emb = embeds_dev; p.sg = sg_dev; p.items = items_dev; p.neg = neg_dev; p.item_out = item_out_dev;
  p.R = R; p.C = C; p.T = T > 0 ? T : 1; p.F = F; p.I = I; p.NE = NE; p.ld = max_neg + 1;
  const hipStream_t s = (hipStream_t)stream;
  if (I > 0) HIP_TRY(sf_launch(sf_clp_items_kernel, dim3((unsigned)I), dim3(256), (size_t)2 * p.ld * 4, s, p));
  HIP_TRY(sf_launch(sf_clp_finish_kernel, dim3(1), dim3(64), 0, s, (const float*)item_out_dev, I, losses_dev));
  return SF_OK;
}

extern "C" size_t sf_op_clp_backward_workspace_bytes(int I, int T, int F, int C) {
  if (I < 0 || T < 0 || F < 1 || C < 1) return 0;
  return 2 * clp_align((size_t)(I > 0 ? I : 1) * C * sizeof(float));
}

extern "C" int sf_op_clp_backward(const float* embeds_dev, int R, int C, const float* sg_dev, const float* stats_dev, const int32_t* track_rows_dev,
                                  const int32_t* track_items_dev, int T, int F, const int32_t* items_dev, int I, const int32_t* neg_dev, int NE,
                                  int max_neg, const int32_t* row_start_dev, const int32_t* row_items_dev, const float* item_out_dev,
                                  const float* upstream_dev, float* grad_embeds_dev, void* workspace, size_t workspace_bytes, sf_stream stream) {
  const char* who = "sf_op_clp_backward";
  if (!embeds_dev || !grad_embeds_dev || !upstream_dev || !workspace) return sf_set_err(SF_ERR_INVALID, "%s: null buffer", who);
  SF_TRY(clp_shape(who, R, C, T, F));
  SF_TRY(clp_items_shape(who, I, NE, max_neg));
  if (I > 0 && (!sg_dev || !stats_dev || !track_rows_dev || !track_items_dev || !items_dev || !row_start_dev || !item_out_dev || T < 1 ||
                (NE > 0 && (!neg_dev || !row_items_dev))))
    return sf_set_err(SF_ERR_INVALID, "%s: null buffer", who);
  SF_TRY(sf_check_workspace(who, "sf_op_clp_backward_workspace_bytes", workspace, workspace_bytes, sf_op_clp_backward_workspace_bytes(I, T, F, C)));
  const hipStream_t s = (hipStream_t)stream;
  if (I == 0) {                                                // no item: every row is exactly zero
    HIP_TRY(hipMemsetAsync(grad_embeds_dev, 0, (size_t)R * C * sizeof(float), s));
    return SF_OK;
  }
  float* ga = (float*)workspace;
  float* gp = (float*)((char*)workspace + clp_align((size_t)I * C * sizeof(float)));
  ClpItemArgs q = {};
  q.emb = embeds_dev; q.sg = sg_dev; q.items = items_dev; q.neg = neg_dev; q.row_start = row_start_dev; q.row_items = row_items_dev; q.up = upstream_dev;
  q.item_out = const_cast<float*>(item_out_dev); q.ga = ga; q.gp = gp; q.grad = grad_embeds_dev;
  q.R = R; q.C = C; q.T = T; q.F = F; q.I = I; q.NE = NE; q.ld = max_neg + 1;
  HIP_TRY(sf_launch(sf_clp_item_bwd_kernel, dim3((unsigned)I), dim3(256), 0, s, q));
  HIP_TRY(sf_launch(sf_clp_neg_bwd_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, s, q));
  ClpTrackArgs p = {};
  p.emb = embeds_dev; p.sg_in = sg_dev; p.stats_in = stats_dev; p.track_rows = track_rows_dev; p.track_items = track_items_dev; p.items = items_dev;
  p.ga = ga; p.gp = gp; p.grad = grad_embeds_dev; p.R = R; p.C = C; p.F = F; p.I = I;
  const size_t lds = (3 * (size_t)F * C + (size_t)F * F + 5 * (size_t)F + 4) * 4;
  HIP_TRY(sf_launch_big_lds(sf_clp_track_bwd_kernel, dim3((unsigned)T), dim3(256), lds, s, p));
  return SF_OK;
}
