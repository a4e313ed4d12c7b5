// Single operators of the forward behind the C ABI, for the parity tests: LayerNorm, one Linear from fp32 operands, one GEMM of a
// named family on the caller's planes, one attention call.  They know the kernels' launchers (sf_common.h), not the encoder.
#include "sf_handle.h"

#include <cmath>
#include <cstring>

__global__ void sf_combine_kernel(const bf16_t* hi, const bf16_t* lo, float* out, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    out[i] = bf2f(hi[i]) + (lo ? bf2f(lo[i]) : 0.f);
}

extern "C" int sf_op_layernorm(const float* x, const float* gamma, const float* beta, float* y, int rows, int D,
                               float eps, sf_stream stream) {
  HIP_TRY(sf_launch_layernorm(x, gamma, beta, y, nullptr, nullptr, rows, D, eps, (hipStream_t)stream));
  return SF_OK;
}

extern "C" size_t sf_op_linear_workspace_bytes(int M, int N, int K) {
  return ((size_t)M * K * 2 + (size_t)N * K * 2 + (size_t)M * N * 2) * 2 + 4096;
}

extern "C" int sf_op_linear(const float* x, const float* w, const float* b, const float* resid, float alpha, int gelu,
                            float* y, int M, int N, int K, int compute, void* workspace, size_t workspace_bytes,
                            sf_stream stream) {
  if (workspace_bytes < sf_op_linear_workspace_bytes(M, N, K)) return sf_set_err(SF_ERR_WORKSPACE, "workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const bool split = compute == SF_COMPUTE_BF16X3;
  SfCarver c(workspace, split, true);      // (the size does not depend on the mode)
  const SfPlanes xp = c.planes((size_t)M * K), wp = c.planes((size_t)N * K), op = c.planes((size_t)M * N);
  HIP_TRY(sf_launch_split(x, xp.hi, xp.lo, (size_t)M * K, s));
  HIP_TRY(sf_launch_split(w, wp.hi, wp.lo, (size_t)N * K, s));
  SfGemmArgs g;
  memset(&g, 0, sizeof(g));
  g.a_hi = xp.hi; g.a_lo = xp.lo; g.w_hi = wp.hi; g.w_lo = wp.lo; g.bias = b;
  g.M = M; g.N = N; g.K = K; g.ldc = N; g.alpha = alpha; g.resid = resid; g.act = 0;
  if (gelu) {
    g.epi = SF_EPI_ACT_BF16; g.out_hi = op.hi; g.out_lo = op.lo;
    HIP_TRY(sf_launch_gemm(g, split, s));
    HIP_TRY(sf_launch(sf_combine_kernel, dim3(1024), dim3(256), 0, s, op.hi, op.lo, y, (size_t)M * N));
  } else {
    g.epi = resid ? SF_EPI_RESID_F32 : SF_EPI_F32; g.out_f32 = y;
    HIP_TRY(sf_launch_gemm(g, split, s));
  }
  return SF_OK;
}

// One forward GEMM with every field of SfGemmArgs the forward sets, on the operand planes as given: the parity tests' way to each
// family and epilogue alone.  Everything the host can check is checked before anything is launched; a named family launches only what
// its own sf_gemm_*_supported accepts.
static const char* gemm_family_name(int f) {
  static const char* const names[] = {"none", "skinny", "tile", "panel", "256^2", "128^2", "256-column + 128-column tail", "lab pipe", "lab pp"};
  return f >= 0 && f <= 8 ? names[f] : "?";
}
extern "C" int sf_op_gemm(const sf_gemm_desc* d, int family, int* family_taken, sf_stream stream) {
  if (family_taken) *family_taken = SF_GEMM_FAM_NONE;
  if (!d) return sf_set_err(SF_ERR_INVALID, "sf_op_gemm: null descriptor");
  if (family < 0 || family > SF_GEMM_FAM_G128) return sf_set_err(SF_ERR_INVALID, "sf_op_gemm: family %d is not one of 0 (dispatch) .. 5", family);
  const bool split = d->split != 0;
  if (d->M <= 0 || d->N <= 0 || d->K <= 0) return sf_set_err(SF_ERR_INVALID, "sf_op_gemm: bad shape M=%d N=%d K=%d", d->M, d->N, d->K);
  if (d->ldc < d->N) return sf_set_err(SF_ERR_INVALID, "sf_op_gemm: ldc %d < N %d", d->ldc, d->N);
  if (!d->a_hi || !d->w_hi) return sf_set_err(SF_ERR_INVALID, "sf_op_gemm: a_hi and w_hi are required");
  if (split && (!d->a_lo || !d->w_lo)) return sf_set_err(SF_ERR_INVALID, "sf_op_gemm: split needs a_lo and w_lo");
  if (!split && (d->a_lo || d->w_lo)) return sf_set_err(SF_ERR_INVALID, "sf_op_gemm: a_lo / w_lo given without split");
  if (d->act < 0 || d->act > 2) return sf_set_err(SF_ERR_INVALID, "sf_op_gemm: act %d is not 0 (erf GELU), 1 (tanh GELU) or 2 (ReLU)", d->act);
  if (d->resid_mod < 0) return sf_set_err(SF_ERR_INVALID, "sf_op_gemm: resid_mod %d < 0", d->resid_mod);
  if (d->resid_mod > 0 && !d->resid) return sf_set_err(SF_ERR_INVALID, "sf_op_gemm: resid_mod needs the fp32 resid table");
  if ((d->resid_hi != nullptr) != (d->resid_lo != nullptr)) return sf_set_err(SF_ERR_INVALID, "sf_op_gemm: resid_hi and resid_lo come together");
  if (d->resid_lo2 && !d->resid_hi) return sf_set_err(SF_ERR_INVALID, "sf_op_gemm: resid_lo2 needs resid_hi and resid_lo");
  if (d->resid && d->resid_hi) return sf_set_err(SF_ERR_INVALID, "sf_op_gemm: resid and resid_hi / resid_lo are two forms of one operand: give one");
  if (d->out_lo && !d->out_hi) return sf_set_err(SF_ERR_INVALID, "sf_op_gemm: out_lo needs out_hi");
  if (d->out_lo2 && !d->out_lo) return sf_set_err(SF_ERR_INVALID, "sf_op_gemm: out_lo2 needs out_hi and out_lo");
  if (!d->ln_inkernel && (d->ln_stats != nullptr) != (d->ln_s != nullptr))
    return sf_set_err(SF_ERR_INVALID, "sf_op_gemm: ln_stats and ln_s come together");
  if (d->ln_inkernel && !d->ln_s) return sf_set_err(SF_ERR_INVALID, "sf_op_gemm: ln_inkernel needs ln_s");
  if (d->ln_inkernel && d->ln_stats) return sf_set_err(SF_ERR_INVALID, "sf_op_gemm: ln_inkernel and ln_stats are two forms of one fold: give one");
  if ((d->ln_stats || d->ln_inkernel) && d->ln_stats_out) return sf_set_err(SF_ERR_INVALID, "sf_op_gemm: a fold consumer does not produce statistics");
  if (d->grp_rows < 0 || (d->grp_rows > 0 && (d->grp_stride < d->grp_rows || d->grp_off < 0)))
    return sf_set_err(SF_ERR_INVALID, "sf_op_gemm: row remap grp_rows=%d grp_stride=%d grp_off=%d (stride >= rows > 0, off >= 0)", d->grp_rows, d->grp_stride, d->grp_off);
  switch (d->epi) {
    case SF_EPI_F32:
      if (!d->out_f32) return sf_set_err(SF_ERR_INVALID, "sf_op_gemm: SF_EPI_F32 needs out_f32");
      break;
    case SF_EPI_BF16: case SF_EPI_ACT_BF16:
      if (!d->out_hi) return sf_set_err(SF_ERR_INVALID, "sf_op_gemm: a bf16 epilogue needs out_hi");
      break;
    case SF_EPI_RESID_F32:
      if (!d->resid && !d->resid_hi) return sf_set_err(SF_ERR_INVALID, "sf_op_gemm: SF_EPI_RESID_F32 needs resid or resid_hi / resid_lo");
      if (d->resid && !d->out_f32) return sf_set_err(SF_ERR_INVALID, "sf_op_gemm: an fp32 residual needs out_f32");
      if (d->resid_hi && (!d->out_hi || !d->out_lo)) return sf_set_err(SF_ERR_INVALID, "sf_op_gemm: a plane-form residual needs out_hi and out_lo");
      break;
    case SF_EPI_EMBED_F32:
      if (!d->out_f32 || !d->pos || !d->time_rows || d->Np <= 0 || d->Tn <= 0)
        return sf_set_err(SF_ERR_INVALID, "sf_op_gemm: SF_EPI_EMBED_F32 needs out_f32, pos, time_rows, Np > 0 and Tn > 0");
      break;
    default: return sf_set_err(SF_ERR_INVALID, "sf_op_gemm: unknown epilogue %d", d->epi);
  }
  if (d->epi != SF_EPI_RESID_F32 && (d->resid || d->resid_hi)) return sf_set_err(SF_ERR_INVALID, "sf_op_gemm: a residual is given to epilogue %d", d->epi);
  if (d->ln_stats_out && !d->out_hi) return sf_set_err(SF_ERR_INVALID, "sf_op_gemm: ln_stats_out comes with the bf16 plane out_hi the consumer reads");
  SfGemmArgs g;
  memset(&g, 0, sizeof(g));
  g.a_hi = d->a_hi; g.a_lo = d->a_lo; g.w_hi = d->w_hi; g.w_lo = d->w_lo; g.bias = d->bias;
  g.M = d->M; g.N = d->N; g.K = d->K; g.epi = d->epi; g.act = d->act; g.alpha = d->alpha;
  g.resid = d->resid; g.resid_mod = d->resid_mod; g.resid_hi = d->resid_hi; g.resid_lo = d->resid_lo; g.resid_lo2 = d->resid_lo2;
  g.pos = d->pos; g.time_rows = d->time_rows; g.Np = d->Np; g.Tn = d->Tn;
  g.out_f32 = d->out_f32; g.out_hi = d->out_hi; g.out_lo = d->out_lo; g.out_lo2 = d->out_lo2; g.ldc = d->ldc;
  g.grp_rows = d->grp_rows; g.grp_stride = d->grp_stride; g.grp_off = d->grp_off;
  g.ln_stats_out = d->ln_stats_out; g.ln_stats = d->ln_stats; g.ln_s = d->ln_s; g.ln_eps = d->ln_eps;
  g.ln_stats_wide = d->ln_stats_wide; g.ln_inkernel = d->ln_inkernel;
  SfGemmFamily fam = SF_GEMM_FAM_NONE;
  if (family == 0) {
    fam = sf_gemm_family(g, split);
    if (fam == SF_GEMM_FAM_NONE) return sf_set_err(SF_ERR_INVALID, "sf_op_gemm: no GEMM family takes this call");
  } else {
    bool ok = false;
    switch (family) {
      case SF_GEMM_FAM_SKINNY: ok = sf_gemm_skinny_supported(g, split); break;
      case SF_GEMM_FAM_TILE: ok = sf_gemm_tile_supported(g, split); break;
      case SF_GEMM_FAM_PANEL: ok = sf_gemm_panel_supported(g, split); break;
      case SF_GEMM_FAM_G256: ok = sf_gemm256_supported(g, split); break;
      default: ok = sf_gemm128_supported(g, split); break;
    }
    if (!ok) return sf_set_err(SF_ERR_INVALID, "sf_op_gemm: the %s family does not take this call (its sf_gemm_*_supported says no)", gemm_family_name(family));
    fam = (SfGemmFamily)family;
  }
  // fields that only some kernels read: the others would ignore them (or read a null buffer in their place), so the call is refused
  const bool p256 = fam == SF_GEMM_FAM_PANEL || fam == SF_GEMM_FAM_G256;
  const char* stray = nullptr;
  if (g.resid_mod > 0 && fam != SF_GEMM_FAM_PANEL) stray = "resid_mod (panel kernel only)";
  else if (g.resid_hi && !p256) stray = "resid_hi / resid_lo (panel and 256^2 kernels only)";
  else if ((g.resid_lo2 || g.out_lo2) && fam != SF_GEMM_FAM_G256) stray = "resid_lo2 / out_lo2 (256^2 kernel only)";
  else if (g.ln_stats && fam != SF_GEMM_FAM_G256) stray = "ln_stats (256^2 kernel only)";
  else if (g.ln_stats_out && !p256 && fam != SF_GEMM_FAM_TILE) stray = "ln_stats_out (tile, panel and 256^2 kernels only)";
  else if (g.ln_inkernel && fam != SF_GEMM_FAM_SKINNY && fam != SF_GEMM_FAM_TILE) stray = "ln_inkernel (skinny and tile kernels only)";
  else if (g.grp_rows > 0 && (fam == SF_GEMM_FAM_PANEL || fam == SF_GEMM_FAM_TILE) && g.epi != SF_EPI_BF16 && g.epi != SF_EPI_ACT_BF16) stray = "the row remap (not on this kernel's fp32 epilogues)";
  else if ((fam == SF_GEMM_FAM_G128 || fam == SF_GEMM_FAM_COLSPLIT) && !sf_gemm128_supported(g, split)) stray = "a field the 128^2 kernel does not read";
  else if (fam == SF_GEMM_FAM_SKINNY && g.epi == SF_EPI_RESID_F32 && !g.resid) stray = "a plane-form residual";
  if (stray) return sf_set_err(SF_ERR_INVALID, "sf_op_gemm: the %s family does not read %s", gemm_family_name(fam), stray);
  HIP_TRY(sf_launch_gemm_family(fam, g, split, (hipStream_t)stream));
  if (family_taken) *family_taken = (int)fam;
  return SF_OK;
}

extern "C" size_t sf_op_attention_workspace_bytes(int groups, int L, int heads, int head_dim) {
  const size_t rows = (size_t)groups * L, D = (size_t)heads * head_dim;
  return rows * 3 * D * 2 * 2 + rows * D * 2 * 2 + 4096;     // qkv hi (+ lo) planes, ctx hi + lo
}

// The arguments of sf_op_attention's kernel call and where its workspace pieces lie: shared with sf_op_spatial_attention_plan, which
// passes no buffers (every pointer is then null, the offsets between them as in a real call), so the query cannot drift from the call.
struct OpAttn {
  SfAttnArgs a;               // everything but the layout's own fields (spatial: N, frames; temporal: the T* fields)
  bf16_t *qb, *ql;            // bf16 rows / lo plane of qkv, filled by sf_launch_split when `split`
  bool split;
};
static OpAttn op_attention_args(const float* qkv, void* workspace, int groups, int L, int heads, int head_dim, bool acc, bool temporal_layout,
                                bool probs) {
  const int D = heads * head_dim;
  const size_t rows = (size_t)groups * L;
  SfCarver c(workspace, acc, true);      // ctx: hi + lo bytes in both modes, the lo plane handed out in the accurate mode
  const SfPlanes cp = c.planes(rows * D);
  OpAttn o;
  o.qb = c.take<bf16_t>(rows * 3 * D);
  const size_t qb_off = c.off;
  const bool planes = acc && head_dim == 64 && (temporal_layout ? sf_temporal_planes_ok(L, L) : sf_spatial_planes_ok(L, probs));
  o.ql = planes ? c.lo(rows * 3 * D) : nullptr;      // (planes: accurate mode only)
  o.split = !acc || planes;
  const void* base = o.split ? (const void*)o.qb : (const void*)qkv;
  const size_t esz = o.split ? 2 : 4;
  SfAttnArgs& a = o.a;
  memset(&a, 0, sizeof(a));
  a.q = base; a.k = (const char*)base + (size_t)D * esz; a.v = (const char*)base + (size_t)2 * D * esz;
  a.in_is_f32 = acc && !planes; a.lo_plane_off = planes ? (long long)((c.off - qb_off) / sizeof(bf16_t)) : 0;      // = ql - qb: two pieces of one size, ends as far apart as starts
  a.row_pitch_q = 3 * D; a.row_pitch_kv = 3 * D; a.heads = heads; a.scale = 1.0f / sqrtf((float)head_dim);
  a.ctx_hi = cp.hi; a.ctx_lo = cp.lo; a.D = D; a.head_dim = head_dim;
  return o;
}

extern "C" int sf_op_spatial_attention_plan(int frames, int N, int heads, int head_dim, int compute, int probs, float dropout, int* route,
                                            int* qsplit, size_t* lds) {
  if (head_dim < 8 || head_dim > 128 || head_dim % 8) return sf_set_err(SF_ERR_INVALID, "head_dim must be a multiple of 8 in 8..128");
  static float probs_wanted;             // the plan only asks whether a.probs is null
  const bool acc = compute == SF_COMPUTE_BF16X3;
  SfAttnArgs a = op_attention_args(nullptr, nullptr, frames, N, heads, head_dim, acc, false, probs != 0).a;
  a.N = N; a.frames = frames;
  if (probs) a.probs = &probs_wanted;
  a.drop = sf_drop_make(dropout, 0u, 0u);
  const SfSpatialPlan pl = sf_spatial_plan(a, acc);
  if (route) *route = (int)pl.route;
  if (qsplit) *qsplit = pl.qsplit;
  if (lds) *lds = pl.lds;
  return SF_OK;
}

extern "C" int sf_op_attention(const float* qkv, float* ctx, int groups, int L, int heads, int head_dim, int causal,
                               int temporal_layout, int N_tokens, int compute, void* workspace, size_t workspace_bytes,
                               sf_stream stream) {
  if (head_dim < 8 || head_dim > 128 || head_dim % 8) return sf_set_err(SF_ERR_INVALID, "head_dim must be a multiple of 8 in 8..128");
  if (workspace_bytes < sf_op_attention_workspace_bytes(groups, L, heads, head_dim)) return sf_set_err(SF_ERR_WORKSPACE, "workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const bool acc = compute == SF_COMPUTE_BF16X3;
  const size_t rows = (size_t)groups * L;
  const OpAttn o = op_attention_args(qkv, workspace, groups, L, heads, head_dim, acc, temporal_layout != 0, false);
  if (o.split) HIP_TRY(sf_launch_split(qkv, o.qb, o.ql, rows * 3 * o.a.D, s));
  SfAttnArgs a = o.a;
  if (temporal_layout) {
    // rows are [B, L, N_tokens, 3D] with groups = B * N_tokens sequences of length L
    if (N_tokens <= 0 || groups % N_tokens) return sf_set_err(SF_ERR_INVALID, "groups must be a multiple of N_tokens");
    a.N = N_tokens; a.B = groups / N_tokens; a.Tq = L; a.Tk = L; a.Tcap = L; a.t_past = 0; a.causal = causal;
    a.Tq_cap = L; a.q_t0 = 0;
    HIP_TRY(sf_launch_temporal_attention(a, acc, s));
  } else {
    if (causal) return sf_set_err(SF_ERR_INVALID, "the spatial layout has no causal variant");
    a.N = L; a.frames = groups;
    HIP_TRY(sf_launch_spatial_attention(a, acc, s));
  }
  HIP_TRY(sf_launch(sf_combine_kernel, dim3(1024), dim3(256), 0, s, a.ctx_hi, a.ctx_lo, ctx, rows * a.D));
  return SF_OK;
}

// Temporal attention over a KV-cache, alone: the streaming step, chunked prefill, the device-side position and the ragged call's table,
// on a cache the CALLER built.  The cache is converted to what the mode keeps in a real stream (bf16 rows; the accurate mode reads the
// caller's fp32 rows) and the arguments are filled as the encoder's layer fills them (forward_layer, sf_encoder.hip).
extern "C" size_t sf_op_attention_cached_workspace_bytes(int slabs, int cap, int N_tokens, int heads, int head_dim, int B, int Tq) {
  const size_t D = (size_t)heads * head_dim;
  return (size_t)slabs * cap * N_tokens * 3 * D * 2 + (size_t)B * Tq * N_tokens * D * 2 * 2 + 4096;      // bf16 cache rows, ctx hi + lo
}

extern "C" int sf_op_attention_cached(const float* cache, float* ctx, int slabs, int cap, int N_tokens, int heads, int head_dim, int compute,
                                      int B, int Tq, int Tk, int q_t0, int t_past, int causal, const int* pos_dev,
                                      const sf_stream_slot* tab, int* route_out, int* waves_out, void* workspace, size_t workspace_bytes,
                                      sf_stream stream) {
  static_assert(sizeof(sf_stream_slot) == sizeof(SfStreamSlot), "sf_stream_slot is SfStreamSlot");
  if (route_out) *route_out = SF_TROUTE_NONE;
  if (waves_out) *waves_out = 0;
  if (!cache || !ctx || ((uintptr_t)cache & 15) || ((uintptr_t)ctx & 15)) return sf_set_err(SF_ERR_INVALID, "sf_op_attention_cached: cache and ctx are 16-byte aligned device buffers");
  if (head_dim < 8 || head_dim > 128 || head_dim % 8) return sf_set_err(SF_ERR_INVALID, "sf_op_attention_cached: head_dim must be a multiple of 8 in 8..128");
  if (compute != SF_COMPUTE_BF16 && compute != SF_COMPUTE_BF16X3) return sf_set_err(SF_ERR_INVALID, "sf_op_attention_cached: compute %d is not bf16 (0) or bf16x3 (1)", compute);
  if (slabs <= 0 || cap <= 0 || N_tokens <= 0 || heads <= 0 || B <= 0 || Tq <= 0 || Tk <= 0)
    return sf_set_err(SF_ERR_INVALID, "sf_op_attention_cached: bad shape slabs=%d cap=%d N_tokens=%d heads=%d B=%d Tq=%d Tk=%d", slabs, cap, N_tokens, heads, B, Tq, Tk);
  if (q_t0 < 0 || q_t0 + Tq > cap) return sf_set_err(SF_ERR_INVALID, "sf_op_attention_cached: query rows q_t0 %d .. + Tq %d leave the cache (cap %d)", q_t0, Tq, cap);
  if (Tk > cap) return sf_set_err(SF_ERR_INVALID, "sf_op_attention_cached: Tk %d > cap %d", Tk, cap);
  if (t_past < 0) return sf_set_err(SF_ERR_INVALID, "sf_op_attention_cached: t_past %d < 0", t_past);
  if (tab && pos_dev) return sf_set_err(SF_ERR_INVALID, "sf_op_attention_cached: tab and pos_dev are two forms of one position: give one");
  if ((tab || pos_dev) && Tq != 1) return sf_set_err(SF_ERR_INVALID, "sf_op_attention_cached: tab / pos_dev serve the single-query kernels (Tq %d != 1)", Tq);
  if (tab ? B > SF_MAX_CALL_STREAMS : B > slabs)
    return sf_set_err(SF_ERR_INVALID, "sf_op_attention_cached: B %d > %d (%s)", B, tab ? SF_MAX_CALL_STREAMS : slabs, tab ? "entries of a table" : "slabs");
  if (workspace_bytes < sf_op_attention_cached_workspace_bytes(slabs, cap, N_tokens, heads, head_dim, B, Tq)) return sf_set_err(SF_ERR_WORKSPACE, "workspace too small");
  hipStream_t s = (hipStream_t)stream;
  // the device-side position is the caller's: every row it names is checked before a kernel follows it
  if (tab || pos_dev) {
    SfStreamSlot host[SF_MAX_CALL_STREAMS];
    int nent = B;
    if (tab) {
      HIP_TRY(hipMemcpy(host, tab, sizeof(SfStreamSlot) * B, hipMemcpyDeviceToHost));
    } else {
      int two[2];
      HIP_TRY(hipMemcpy(two, pos_dev, sizeof(two), hipMemcpyDeviceToHost));
      host[0].stream = 0; host[0].t_row = 0; host[0].slot = two[0]; host[0].tk = two[1];
      nent = 1;
    }
    for (int b = 0; b < nent; ++b) {
      const SfStreamSlot& e = host[b];
      if (e.stream < 0 || e.stream >= slabs || e.slot < 0 || e.slot >= cap || e.tk < 1 || e.tk > Tk)
        return sf_set_err(SF_ERR_INVALID, "sf_op_attention_cached: device position %d {stream %d, slot %d, tk %d} outside slabs %d, cap %d, Tk %d", b, e.stream,
                          e.slot, e.tk, slabs, cap, Tk);
    }
  }
  const bool acc = compute == SF_COMPUTE_BF16X3;
  const int D = heads * head_dim;
  const size_t rows = (size_t)B * Tq * N_tokens, cells = (size_t)slabs * cap * N_tokens * 3 * D;
  SfCarver c(workspace, acc, true);
  const SfPlanes cp = c.planes(rows * D);
  bf16_t* qb = c.take<bf16_t>(cells);
  const void* base = cache;
  size_t esz = 4;
  if (!acc) {
    HIP_TRY(sf_launch_split(cache, qb, nullptr, cells, s));
    base = qb;
    esz = 2;
  }
  SfAttnArgs a;
  memset(&a, 0, sizeof(a));
  a.q = base; a.k = (const char*)base + (size_t)D * esz; a.v = (const char*)base + (size_t)2 * D * esz;
  a.in_is_f32 = acc; a.lo_plane_off = 0;
  a.row_pitch_q = 3 * D; a.row_pitch_kv = 3 * D; a.heads = heads; a.scale = 1.0f / sqrtf((float)head_dim); a.head_dim = head_dim;
  a.N = N_tokens; a.ctx_hi = cp.hi; a.ctx_lo = cp.lo; a.D = D;
  a.B = B; a.Tq = Tq; a.Tk = Tk; a.Tcap = cap; a.t_past = t_past;
  a.causal = causal; a.Tq_cap = cap; a.q_t0 = q_t0;
  a.pos_dev = pos_dev; a.tab = reinterpret_cast<const SfStreamSlot*>(tab);
  const SfTemporalRoute r = sf_temporal_route(a, acc);
  if (r == SF_TROUTE_NONE) return sf_set_err(SF_ERR_INVALID, "sf_op_attention_cached: no temporal attention kernel takes this call");
  const bool single = (r >= SF_TROUTE_DECODE_F32_KP1 && r <= SF_TROUTE_DECODE_BF16_KP4) || r == SF_TROUTE_GENERIC;
  if ((tab || pos_dev) && !single)
    return sf_set_err(SF_ERR_INVALID, "sf_op_attention_cached: route %d does not read tab / pos_dev (single-query and generic kernels only)", (int)r);
  HIP_TRY(sf_launch_temporal_route(r, a, s));
  HIP_TRY(sf_launch(sf_combine_kernel, dim3(1024), dim3(256), 0, s, cp.hi, cp.lo, ctx, rows * D));
  if (route_out) *route_out = (int)r;
  if (waves_out) *waves_out = sf_temporal_route_waves(r, a);
  return SF_OK;
}
