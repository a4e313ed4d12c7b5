// Bench hooks behind the C ABI (bench.py's roofline rows and launch floor): the forward's own GEMM and attention launches, and a graph
// of empty kernels, timed with HIP events on the caller's stream.
#include "sf_encoder.h"

#include <cstring>

// `launch` once untimed, then `iters` times between two events on `s`: *mean_ms = elapsed / iters.  Returns the first error; the
// events are destroyed on every path.
template <typename Launch>
static hipError_t sf_time_launches(hipStream_t s, int iters, Launch&& launch, float* mean_ms) {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipError_t err = hipEventCreate(&e0);
  if (err == hipSuccess) err = hipEventCreate(&e1);
  if (err == hipSuccess) err = launch();      // warm
  if (err == hipSuccess) err = hipEventRecord(e0, s);
  for (int i = 0; i < iters && err == hipSuccess; ++i) err = launch();
  if (err == hipSuccess) err = hipEventRecord(e1, s);
  if (err == hipSuccess) err = hipEventSynchronize(e1);
  float ms = 0.f;
  if (err == hipSuccess) err = hipEventElapsedTime(&ms, e0, e1);
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (err == hipSuccess) *mean_ms = ms / iters;
  return err;
}

// ------------------------------------------------------------------------------------------------
// bench hook: time the dominant GEMM with HIP events on the caller's stream
// ------------------------------------------------------------------------------------------------
extern "C" int sf_bench_gemm(sf_encoder* e, int M, int which, int iters, void* workspace, size_t workspace_bytes,
                             sf_stream stream, float* mean_ms_out, double* flops_out) {
  if (!e || !e->finalized || e->layers.empty()) return sf_set_err(SF_ERR_STATE, "encoder not finalized");
  if (iters <= 0 || M <= 0 || !workspace || !mean_ms_out) return sf_set_err(SF_ERR_INVALID, "bad argument");
  const DevLayer& l = e->layers[0];
  // which 0..3 = MLP-up, MLP-down, qkv, attention out-proj with the epilogues the forward gives them; 4 / 5 = out-proj / MLP-down PLAIN (bf16
  // output, no residual, no row sums): the like-for-like partner of a vendor-library GEMM (bench.py roofline.yardstick_tflops)
  const bool plain = which == 4 || which == 5;
  if (plain) which = which == 4 ? 3 : 1;
  const DevLinear* lin = which == 0 ? &l.up : which == 1 ? &l.down : which == 2 ? &l.s_qkv : &l.s_out;
  const bool acc = e->compute == SF_COMPUTE_BF16X3;
  const int epi = plain ? (acc ? SF_EPI_F32 : SF_EPI_BF16) : which == 0 ? SF_EPI_ACT_BF16 : which == 2 ? (acc ? SF_EPI_F32 : SF_EPI_BF16) : SF_EPI_RESID_F32;
  // bf16 mode at BASELINE-sized M: the residual projections as the forward launches them — hi + lo planes in and out, LayerNorm
  // row sums of the next Linear (ForwardPlan's `fold + pm`, by the plan's own rule); fp32 residual + bf16 copy otherwise
  const bool pm = epi == SF_EPI_RESID_F32 && resid_planes_at(e, M);
  SfCarver c(workspace, acc || pm, true);      // pm: the residual stream has its lo plane in bf16 mode too
  const SfPlanes ap = c.planes((size_t)M * lin->K);
  SfPlanes op = c.planes((size_t)M * lin->N);
  float* of = c.take<float>((size_t)M * lin->N);
  if (c.off > workspace_bytes) return sf_set_err(SF_ERR_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, c.off);
  hipStream_t s = (hipStream_t)stream;
  if (acc && epi == SF_EPI_RESID_F32) op.hi = nullptr;     // the accurate mode keeps no bf16 copy of the residual (no LayerNorm fold)
  float* st = pm ? c.take<float>((size_t)M * 8) : nullptr;
  if (c.off > workspace_bytes) return sf_set_err(SF_ERR_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, c.off);
  if (st) HIP_TRY(hipMemsetAsync(st, 0, (size_t)M * 8 * sizeof(float), (hipStream_t)stream));
  SfGemmArgs g = linear_args(e, *lin, ap.hi, ap.lo, M, epi, acc);
  g.alpha = 0.f; g.out_hi = op.hi; g.out_lo = op.lo;
  if (pm) { g.resid_hi = op.hi; g.resid_lo = op.lo; g.ln_stats_out = st; }
  else { g.out_f32 = of; g.resid = of; }
  HIP_TRY(sf_time_launches(s, iters, [&]() { return sf_launch_gemm(g, acc, s); }, mean_ms_out));
  if (flops_out) *flops_out = 2.0 * M * (double)lin->N * (double)lin->K;
  return SF_OK;
}

extern "C" int sf_bench_attention(sf_encoder* e, int B, int T, int which, int iters, void* workspace,
                                  size_t workspace_bytes, sf_stream stream, float* mean_ms_out, double* bytes_out,
                                  double* flops_out) {
  if (!e || !e->finalized) return sf_set_err(SF_ERR_STATE, "encoder not finalized");
  if (iters <= 0 || B <= 0 || T <= 0 || !workspace || !mean_ms_out) return sf_set_err(SF_ERR_INVALID, "bad argument");
  const bool acc = e->compute == SF_COMPUTE_BF16X3;
  const int D = e->D, N = e->N, heads = e->cfg.num_attention_heads;
  const size_t M = (size_t)B * T * N, esz = acc ? 4 : 2;
  SfCarver c(workspace);
  char* qkv = c.take<char>(M * 3 * D * esz);
  bf16_t* ch = c.take<bf16_t>(M * D);
  bf16_t* cl = c.take<bf16_t>(M * D);
  if (c.off > workspace_bytes) return sf_set_err(SF_ERR_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, c.off);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(qkv, 0x3c, M * 3 * D * esz, s));   // finite, non-trivial bit pattern
  SfAttnArgs a;
  memset(&a, 0, sizeof(a));
  a.q = qkv; a.k = qkv + (size_t)D * esz; a.v = qkv + (size_t)2 * D * esz;
  a.in_is_f32 = acc; a.row_pitch_q = 3 * D; a.row_pitch_kv = 3 * D; a.heads = heads; a.scale = 0.125f;
  a.ctx_hi = ch; a.ctx_lo = cl; a.D = D; a.N = N;
  if (which == 0 && acc && sf_spatial_planes_ok(N, false)) {      // what the forward does: hi + lo planes in the fp32 tensor's bytes
    a.k = qkv + (size_t)D * 2; a.v = qkv + (size_t)2 * D * 2;
    a.in_is_f32 = 0; a.lo_plane_off = (long long)M * 3 * D;
  }
  if (which == 1 && acc && sf_temporal_planes_ok(T, T)) {
    a.k = qkv + (size_t)D * 2; a.v = qkv + (size_t)2 * D * 2;
    a.in_is_f32 = 0; a.lo_plane_off = (long long)M * 3 * D;
  }
  if (which == 0) {
    a.frames = B * T;
  } else {
    a.B = B; a.Tq = T; a.Tk = T; a.Tcap = T; a.t_past = 0; a.causal = e->cfg.enable_causal_temporal; a.Tq_cap = T; a.q_t0 = 0;
  }
  auto launch = [&]() { return which == 0 ? sf_launch_spatial_attention(a, acc, s) : sf_launch_temporal_attention(a, acc, s); };
  HIP_TRY(sf_time_launches(s, iters, launch, mean_ms_out));
  if (bytes_out) *bytes_out = (double)M * 3 * D * esz + (double)M * D * 2 * (acc ? 2 : 1);
  if (flops_out) {
    const double L = which == 0 ? N : T;        // 2 matmuls of L x L x 64 per (sequence, head), full (not causal-halved)
    const double seqs = which == 0 ? (double)B * T : (double)B * N;
    *flops_out = seqs * heads * 2.0 * (2.0 * L * L * 64.0);
  }
  return SF_OK;
}

// ------------------------------------------------------------------------------------------------
// launch floor (bench hook): a graph of dependent empty kernels
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sf_null_kernel(int* sink) {
  if (sink && threadIdx.x == 1024) *sink = 0;     // never true: the kernel has no memory traffic
}
extern "C" int sf_bench_launch_floor(int device, int launches, int iters, sf_stream stream, float* us_per_launch_out) {
  if (launches <= 0 || iters <= 0 || !us_per_launch_out) return sf_set_err(SF_ERR_INVALID, "bad argument");
  HIP_TRY(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  hipStream_t cap = nullptr;
  HIP_TRY(hipStreamCreateWithFlags(&cap, hipStreamNonBlocking));
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  hipError_t err = hipStreamBeginCapture(cap, hipStreamCaptureModeThreadLocal);
  if (err == hipSuccess) {
    for (int i = 0; i < launches && err == hipSuccess; ++i) err = sf_launch(sf_null_kernel, dim3(256), dim3(256), 0, cap, (int*)nullptr);
    const hipError_t end = hipStreamEndCapture(cap, &graph);
    if (err == hipSuccess) err = end;
  }
  if (err == hipSuccess) err = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  float ms = 0.f;
  if (err == hipSuccess) {
    // its own loop, not sf_time_launches: the stream is idle when the first record is enqueued (one untimed replay and a synchronise)
    hipEvent_t e0 = nullptr, e1 = nullptr;
    err = hipEventCreate(&e0);
    if (err == hipSuccess) err = hipEventCreate(&e1);
    if (err == hipSuccess) {
      (void)hipGraphLaunch(exec, s);
      (void)hipStreamSynchronize(s);
      (void)hipEventRecord(e0, s);
      for (int i = 0; i < iters; ++i) (void)hipGraphLaunch(exec, s);
      (void)hipEventRecord(e1, s);
      err = hipEventSynchronize(e1);
      (void)hipEventElapsedTime(&ms, e0, e1);
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
  if (exec) (void)hipGraphExecDestroy(exec);
  if (graph) (void)hipGraphDestroy(graph);
  (void)hipStreamDestroy(cap);
  if (err != hipSuccess) return sf_set_err(SF_ERR_HIP, "sf_bench_launch_floor: %s", hipGetErrorString(err));
  *us_per_launch_out = 1e3f * ms / ((float)iters * (float)launches);
  return SF_OK;
}
