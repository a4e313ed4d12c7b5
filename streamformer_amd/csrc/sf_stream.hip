// Streaming (vqa_enc:1316-1392): the KV-cache, parking (kernels: sf_cache_park.hip), the sf_forward_stream* entries and their graphs; a call is a ForwardRequest run by sf_encoder.hip
#include "sf_encoder.h"
#include <set>
#include <tuple>
struct sf_cache {
  sf_encoder* enc = nullptr;
  uint64_t enc_generation = 0;   // packing of the encoder this cache was sized for (element size, device, weights)
  int B = 0, cap = 0, H = 0, W = 0, N = 0;
  std::vector<int> lens;    // frames seen per stream; the lockstep entry points need them level
  int len() const { int m = 0; for (int v : lens) m = v > m ? v : m; return m; }      // the largest (every stream's, when level)
  bool level() const { for (int v : lens) if (v != lens[0]) return false; return true; }
  void advance(int T) { for (int& v : lens) v += T; }
  std::vector<void*> qkv;   // per layer [B, cap, N, 3D] (bf16 or fp32 by compute mode)
  size_t bytes = 0;
  // hipGraph of the per-call launch sequence: everything between the patch extraction (reads the caller's pixels) and the
  // copy-out (writes the caller's outputs) is replayed as one graph launch.  The key names what is compiled into a capture;
  // the entry holds what else it is valid for (the addresses its nodes carry).
  enum GraphKind { PER_POSITION, POSITION_FREE, RAGGED };      // lockstep, several frames per call / lockstep, one frame / named streams
  struct GraphKey {
    int kind = PER_POSITION;
    int rows = 0, T_new = 0;          // row groups (streams) and frames per stream of the call
    int at = 0;                       // PER_POSITION: frames cached; otherwise the key-pass class (key_pass_class)
    int pooler = 0, pixel_kind = 0;   // pooler_output wanted; 0 fp32, 1 bf16, 2 uint8 frames
    bool operator<(const GraphKey& o) const {
      return std::tie(kind, rows, T_new, at, pooler, pixel_kind) < std::tie(o.kind, o.rows, o.T_new, o.at, o.pooler, o.pixel_kind);
    }
  };
  struct GraphEntry {
    hipGraphExec_t exec = nullptr;
    void* ws = nullptr;
    const float* pos = nullptr;
  };
  std::map<GraphKey, GraphEntry> graphs;
  // Keys that have run eagerly once, so that the lazy per-kernel set-up (sf_launch_big_lds: the dynamic-LDS attribute; device queries) of
  // the instances that pass ran has happened before a capture is opened.  The lockstep entry warms once per cache, under kLockstepWarm;
  // the ragged entry once per key (another row count selects other GEMM kernels).  The set-up is per kernel instance: one the warm pass
  // did not run (a temporal or pooling instance of a longer cache, and the same holds for the GEMM families) gets its attribute at its
  // first launch, which may be inside a hipStreamCaptureModeThreadLocal capture; setting the attribute is not a stream operation.
  std::set<GraphKey> warmed;
  hipStream_t cap_stream = nullptr;   // captures are recorded on a private stream (the caller's may be the null stream, which
                                      // cannot capture) and replayed on the caller's
  int policy = 0;                     // 0 = stop at capacity (the reference raises there), 1 = sliding window over the last `cap` frames
  SfStreamParams* dparams = nullptr;  // device block {pixels, outputs, position} of the single-frame graph (one graph for all positions)
  SfStreamSlot* dtable = nullptr;     // behind it: the stream table of a ragged call, SF_MAX_CALL_STREAMS entries (sf_forward_stream_slots)
};

extern "C" int sf_cache_create(sf_encoder* e, int B, int max_frames, int H, int W, sf_cache** out) {
  int N;
  const float* dummy = (const float*)1;
  int rc = check_geometry(e, B, 1, H, W, dummy, &N);
  if (rc) return rc;
  if (!out || max_frames <= 0 || max_frames > 256) return sf_set_err(SF_ERR_INVALID, "max_frames must be in 1..256");
  if (!e->finalized) return sf_set_err(SF_ERR_STATE, "sf_finalize_weights has not run");
  HIP_TRY(hipSetDevice(e->device));
  sf_cache* c = new sf_cache();
  c->enc = e; c->enc_generation = e->generation; c->B = B; c->cap = max_frames; c->H = H; c->W = W; c->N = N;
  c->lens.assign(B, 0);
  const size_t per = (size_t)B * max_frames * N * 3 * e->D * (e->compute == SF_COMPUTE_BF16X3 ? 4 : 2);
  for (int i = 0; i < e->L; ++i) {
    void* p = nullptr;
    hipError_t err = hipMalloc(&p, per);
    if (err != hipSuccess) {
      for (void* q : c->qkv) (void)hipFree(q);
      delete c;
      return sf_set_err(SF_ERR_HIP, "hipMalloc(%zu) for the KV-cache: %s", per, hipGetErrorString(err));
    }
    c->qkv.push_back(p);
  }
  c->bytes = per * e->L;
  // the parameter block, and behind it (256-byte aligned) the stream table of a ragged call
  if (hipMalloc((void**)&c->dparams, 256 + sizeof(SfStreamSlot) * SF_MAX_CALL_STREAMS) != hipSuccess) {
    for (void* q : c->qkv) (void)hipFree(q);
    delete c;
    return sf_set_err(SF_ERR_HIP, "hipMalloc for the stream parameter block failed");
  }
  static_assert(sizeof(SfStreamParams) <= 256, "the stream table sits 256 bytes behind the parameter block");
  c->dtable = reinterpret_cast<SfStreamSlot*>(reinterpret_cast<char*>(c->dparams) + 256);
  *out = c;
  return SF_OK;
}
extern "C" int sf_cache_reset(sf_cache* c) {
  if (!c) return sf_set_err(SF_ERR_INVALID, "null cache");
  c->lens.assign(c->B, 0);
  return SF_OK;
}
extern "C" int sf_cache_reset_stream(sf_cache* c, int stream) {
  if (!c) return sf_set_err(SF_ERR_INVALID, "null cache");
  if (stream < 0 || stream >= c->B) return sf_set_err(SF_ERR_INVALID, "stream %d outside this cache's %d streams", stream, c->B);
  c->lens[stream] = 0;
  return SF_OK;
}
extern "C" int sf_cache_length(const sf_cache* c) { return c ? c->len() : 0; }
extern "C" int sf_cache_stream_length(const sf_cache* c, int stream) { return (c && stream >= 0 && stream < c->B) ? c->lens[stream] : 0; }
extern "C" int sf_cache_set_policy(sf_cache* c, int policy) {
  if (!c || (policy != 0 && policy != 1)) return sf_set_err(SF_ERR_INVALID, "policy must be 0 (stop at capacity) or 1 (sliding window)");
  if (c->len() != 0) return sf_set_err(SF_ERR_STATE, "the policy of a cache is chosen while it is empty");
  c->policy = policy;
  return SF_OK;
}
extern "C" size_t sf_cache_bytes(const sf_cache* c) { return c ? c->bytes : 0; }
static void drop_graphs(sf_cache* c) {
  for (auto& kv : c->graphs)
    if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
  c->graphs.clear();
}
extern "C" void sf_cache_destroy(sf_cache* c) {
  if (!c) return;
  drop_graphs(c);
  if (c->cap_stream) (void)hipStreamDestroy(c->cap_stream);
  for (void* q : c->qkv) (void)hipFree(q);
  if (c->dparams) (void)hipFree(c->dparams);
  delete c;
}
extern "C" int sf_stream_workspace_bytes(sf_encoder* e, const sf_cache* c, int T_new, size_t* out) {
  if (!e || !c || !out || T_new <= 0) return sf_set_err(SF_ERR_INVALID, "bad argument");
  if (c->enc != e || c->enc_generation != e->generation) return sf_set_err(SF_ERR_STATE, "cache does not belong to this encoder's current weight packing");
  *out = carve(e, nullptr, c->B, T_new, c->N, false).bytes;
  return SF_OK;
}
// What the lockstep entry records in sf_cache::warmed: no key of a call equals it, a call has rows >= 1.
static const sf_cache::GraphKey kLockstepWarm = {};

// The cache was created by this encoder, as it is packed now.
static int check_cache_owner(const sf_encoder* e, const sf_cache* c) {
  if (!e || !c || c->enc != e) return sf_set_err(SF_ERR_INVALID, "cache does not belong to this encoder");
  // a handle address can be reused after sf_destroy, and sf_finalize_weights may have changed the compute mode (cache element
  // size) or the device: the generation stamp tells a cache of an earlier packing from a current one
  if (c->enc_generation != e->generation)
    return sf_set_err(SF_ERR_STATE, "cache was created for an earlier weight packing of this encoder (sf_finalize_weights ran since): create a new cache");
  return SF_OK;
}

// ---- parking a stream (kernels: sf_cache_park.hip) -------------------------------------------------------------------------------
static size_t cache_elem_bytes(const sf_encoder* e) { return e->compute == SF_COMPUTE_BF16X3 ? 4 : 2; }
// bytes of the k | v columns of `held` frames over all layers
static size_t stream_blob_bytes(const sf_cache* c, int held) {
  return (size_t)c->enc->L * held * c->N * 2 * c->enc->D * cache_elem_bytes(c->enc);
}
static int check_stream_id(const sf_cache* c, int stream) {
  if (stream < 0 || stream >= c->B) return sf_set_err(SF_ERR_INVALID, "stream %d outside this cache's %d streams (ids are 0 .. %d)", stream, c->B, c->B - 1);
  return SF_OK;
}
extern "C" int sf_cache_stream_blob_bytes(const sf_cache* c, int stream, size_t* out) {
  if (!c || !out) return sf_set_err(SF_ERR_INVALID, "null argument");
  if (int rc = check_stream_id(c, stream)) return rc;
  const int seen = c->lens[stream];
  *out = stream_blob_bytes(c, seen < c->cap ? seen : c->cap);
  return SF_OK;
}
// one launch for up to SF_PARK_MAX_LAYERS layers (every model the library accepts today), further launches beyond
static int park_stream(const sf_encoder* e, const sf_cache* c, int stream, int held, void* blob, bool do_export, hipStream_t s) {
  const size_t esz = cache_elem_bytes(e), row = (size_t)3 * e->D * esz;
  SfParkArgs a;
  memset(&a, 0, sizeof(a));
  a.blob = (char*)blob; a.row_bytes = row; a.kv_off = (size_t)e->D * esz; a.slab_off = (size_t)stream * c->cap * c->N * row;
  a.vpr = (uint32_t)(2 * e->D * esz / 16);
  const size_t nvec = (size_t)held * c->N * a.vpr;
  if (nvec > 0x7fffffffu) return sf_set_err(SF_ERR_CAPACITY, "a stream of %zu bytes per layer is beyond one export launch", nvec * 16);
  a.nvec = (uint32_t)nvec; a.layer_blob_bytes = nvec * 16;
  for (int l0 = 0; l0 < e->L; l0 += SF_PARK_MAX_LAYERS) {
    const int n = e->L - l0 < SF_PARK_MAX_LAYERS ? e->L - l0 : SF_PARK_MAX_LAYERS;
    for (int l = 0; l < n; ++l) a.layer[l] = (char*)c->qkv[l0 + l];
    a.layer0 = l0;
    HIP_TRY(sf_launch_cache_park(a, n, do_export, s));
  }
  return SF_OK;
}
extern "C" int sf_cache_export_stream(sf_encoder* e, sf_cache* c, int stream, void* blob, size_t bytes, sf_cache_stream_meta* meta,
                                      sf_stream s) {
  int rc = check_cache_owner(e, c);
  if (rc) return rc;
  if (!meta) return sf_set_err(SF_ERR_INVALID, "null meta_out");
  if ((rc = check_stream_id(c, stream))) return rc;
  const int seen = c->lens[stream], held = seen < c->cap ? seen : c->cap;
  const size_t need = stream_blob_bytes(c, held);
  if (bytes != need) return sf_set_err(SF_ERR_INVALID, "blob of %zu bytes; stream %d holds %d frames = %zu bytes (sf_cache_stream_blob_bytes)", bytes, stream, held, need);
  if (need && (!blob || ((size_t)blob & 15))) return sf_set_err(SF_ERR_INVALID, "the blob must be a 16-byte aligned device buffer");
  if (need && (rc = park_stream(e, c, stream, held, blob, true, (hipStream_t)s))) return rc;
  memset(meta, 0, sizeof(*meta));
  meta->format = SF_STREAM_BLOB_KV1; meta->compute = e->compute; meta->frames_seen = seen; meta->frames_held = held;
  meta->max_frames = c->cap; meta->policy = c->policy; meta->H = c->H; meta->W = c->W;
  meta->layers = e->L; meta->hidden_size = e->D; meta->patches = c->N; meta->elem_bytes = (int32_t)cache_elem_bytes(e);
  meta->packing = e->fingerprint; meta->blob_bytes = need;
  return SF_OK;
}
extern "C" int sf_cache_import_stream(sf_encoder* e, sf_cache* c, int stream, const void* blob, size_t bytes,
                                      const sf_cache_stream_meta* m, sf_stream s) {
  int rc = check_cache_owner(e, c);
  if (rc) return rc;
  if (!m) return sf_set_err(SF_ERR_INVALID, "null meta");
  if ((rc = check_stream_id(c, stream))) return rc;
  if (m->format != SF_STREAM_BLOB_KV1) return sf_set_err(SF_ERR_INVALID, "format: blob tag 0x%08x is not SF_STREAM_BLOB_KV1", m->format);
  if (m->compute != e->compute)
    return sf_set_err(SF_ERR_INVALID, "compute mode: the stream was parked in mode %d, this encoder is packed for mode %d", m->compute, e->compute);
  if (m->H != c->H || m->W != c->W) return sf_set_err(SF_ERR_INVALID, "resolution: the stream was parked at %dx%d, this cache is %dx%d", m->H, m->W, c->H, c->W);
  if (m->max_frames != c->cap)
    return sf_set_err(SF_ERR_INVALID, "max_frames: the stream was parked from a cache of %d frames, this one holds %d (restoring into another "
                   "capacity is not supported)", m->max_frames, c->cap);
  if (m->policy != c->policy) return sf_set_err(SF_ERR_INVALID, "policy: the stream was parked under policy %d, this cache has policy %d", m->policy, c->policy);
  if (m->layers != e->L || m->hidden_size != e->D || m->patches != c->N || m->elem_bytes != (int32_t)cache_elem_bytes(e))
    return sf_set_err(SF_ERR_INVALID, "geometry: blob of %d layers x %d patches x width %d x %d bytes, cache of %d x %d x %d x %zu", m->layers, m->patches,
                   m->hidden_size, m->elem_bytes, e->L, c->N, e->D, cache_elem_bytes(e));
  if (m->frames_seen < 0 || m->frames_held != (m->frames_seen < c->cap ? m->frames_seen : c->cap) || (c->policy != 1 && m->frames_seen > c->cap))
    return sf_set_err(SF_ERR_INVALID, "frames: %d seen / %d held do not describe a stream of a %d-frame cache", m->frames_seen, m->frames_held, c->cap);
  if (m->packing != e->fingerprint)
    return sf_set_err(SF_ERR_STATE, "packing: the stream was parked by other weights (fingerprint %016llx, this encoder %016llx): its keys and values "
                   "mean nothing here", (unsigned long long)m->packing, (unsigned long long)e->fingerprint);
  const size_t need = stream_blob_bytes(c, m->frames_held);
  if (bytes != need || m->blob_bytes != need)
    return sf_set_err(SF_ERR_INVALID, "byte count: blob of %zu bytes (meta says %llu), %d frames are %zu", bytes, (unsigned long long)m->blob_bytes,
                   m->frames_held, need);
  if (need && (!blob || ((size_t)blob & 15))) return sf_set_err(SF_ERR_INVALID, "the blob must be a 16-byte aligned device buffer");
  if (need && (rc = park_stream(e, c, stream, m->frames_held, const_cast<void*>(blob), false, (hipStream_t)s))) return rc;
  c->lens[stream] = m->frames_seen;      // the next frame's time row, slot and key count follow from it (stream_position)
  return SF_OK;
}

// What the streaming entries share once the cache is known to be the encoder's: the checked arguments of a call of `rows` streams.
struct StreamCall {
  Workspace ws;
  ForwardRequest rq;      // input, geometry and cache filled in; the entry sets the outputs and the position
  hipStream_t s = nullptr;
  int pk = 0;             // pixel kind of sf_launch_patchify
  bool graph_ok = false;  // graphs are not switched off and the caller is not capturing the stream itself
};
// lockstep: the call advances every stream of the cache, which must be level.  positions(): the entry's position refusals; they come
// before the workspace refusal.
template <typename Positions>
static int open_stream_call(sf_encoder* e, sf_cache* c, int rows, int T_new, bool lockstep, const void* pixels, int pixel_dtype,
                            const float* last_hidden, const float* pos_dev, void* workspace, size_t workspace_bytes, sf_stream stream,
                            Positions&& positions, StreamCall* call) {
  int N;
  int rc = check_geometry(e, rows, T_new, c->H, c->W, pos_dev, &N);
  if (rc) return rc;
  if (lockstep && !c->level())
    return sf_set_err(SF_ERR_STATE, "the streams of this cache are at different positions (longest %d frames): advance them with sf_forward_stream_slots "
                   "(stream_ids= in Python), or level them with sf_cache_reset", c->len());
  if (!pixels || !last_hidden || !workspace) return sf_set_err(SF_ERR_INVALID, "null buffer");
  if (pixel_dtype != SF_F32 && pixel_dtype != SF_BF16 && pixel_dtype != SF_U8) return sf_set_err(SF_ERR_INVALID, "pixels must be fp32, bf16 or uint8");
  if ((rc = positions())) return rc;
  call->ws = carve(e, workspace, rows, T_new, N, false);
  if (call->ws.bytes > workspace_bytes) return sf_set_err(SF_ERR_WORKSPACE, "workspace %zu < required %zu bytes", workspace_bytes, call->ws.bytes);
  call->pk = pixel_dtype == SF_U8 ? 2 : (pixel_dtype == SF_BF16 ? 1 : 0);
  call->s = (hipStream_t)stream;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(call->s, &cap);
  call->graph_ok = !sf_sw(SW_DISABLE_STREAM_GRAPH) && cap == hipStreamCaptureStatusNone;
  ForwardRequest& rq = call->rq;
  rq.pixels = pixels; rq.pixel_dtype = pixel_dtype; rq.B = rows; rq.T = T_new; rq.H = c->H; rq.W = c->W; rq.pos_dev = pos_dev;
  rq.layer_tqkv = c->qkv.data(); rq.cap = c->cap; rq.streaming = true;
  return SF_OK;
}

// Position of the first of T_new frames that follow `len` cached ones, or the refusal (stream: the id a ragged call names, -1 for a
// lockstep call).  Sliding window (policy 1, beyond the reference, which raises at num_frames): once the cache is full the new
// frame overwrites the oldest slot, its query sees the last `cap` frames, and frames past the time-embedding table reuse its
// last row (the nearest-neighbour extension modeling:441-447 applies to long clips).
static int stream_position(const sf_cache* c, int len, int T_new, int stream, StreamPos* out) {
  const int nf = c->enc->cfg.num_frames, cap = c->cap;
  if (c->policy == 1 && T_new == 1) {
    *out = {len < nf ? len : nf - 1, len % cap, len + 1 < cap ? len + 1 : cap};
    return SF_OK;
  }
  if (c->policy == 1 && len + T_new > (cap < nf ? cap : nf))
    return sf_set_err(SF_ERR_CAPACITY, "a sliding-window cache that is full (%d of %d frames) advances one frame per call, got %d", len, cap, T_new);
  if (len + T_new > cap)
    return stream < 0 ? sf_set_err(SF_ERR_CAPACITY, "cache holds %d of %d frames; %d more do not fit", len, cap, T_new)
                      : sf_set_err(SF_ERR_CAPACITY, "stream %d holds %d of %d frames; one more does not fit: leave it out of the call, or restart it with "
                                "sf_cache_reset_stream", stream, len, cap);
  if (len + T_new > nf)
    return stream < 0 ? sf_set_err(SF_ERR_CAPACITY, "streaming needs time-embedding row %d but config.num_frames is %d", len + T_new - 1, nf)
                      : sf_set_err(SF_ERR_CAPACITY, "stream %d needs time-embedding row %d but config.num_frames is %d: leave it out of the call, or restart it "
                                "with sf_cache_reset_stream", stream, len + T_new - 1, nf);
  *out = {len, len, len + T_new};
  return SF_OK;
}

// The single-query attention compiles in its number of 64-key passes, 1 / 2 / 4: the only thing about a position that a
// position-free capture fixes (at most three graphs per call shape).
static int key_pass_class(int tk) {
  const int kp = (tk + 63) >> 6;
  return kp <= 1 ? 1 : (kp <= 2 ? 2 : 4);
}
// A key count of the class that this cache can reach: it selects the kernels, which read the live position from the device.
static StreamPos class_position(const sf_cache* c, int kcls) {
  const int nf = c->enc->cfg.num_frames;
  int tk = kcls * 64;
  if (tk > c->cap) tk = c->cap;
  if (c->policy != 1 && tk > nf) tk = nf;
  return {0, 0, tk};
}

// The forward of a position-free call (one frame per stream; ragged: the named streams through the device table): patch matrix
// already extracted by the launch that delivered the parameter block, last_hidden_state written straight into the caller's tensor
// through the block, pooler_output too when the head's row-vector tail runs (<= 4 rows): no staging copy at the end.
static int run_position_free(sf_encoder* e, sf_cache* c, const StreamCall& call, int kcls, bool ragged, bool pooler, hipStream_t on) {
  const StreamPos rep = class_position(c, kcls);
  ForwardRequest rq = call.rq;
  rq.last_hidden = call.ws.lhs_stage; rq.pooler = pooler ? call.ws.pool_stage : nullptr;
  rq.ready = 1; rq.sp = c->dparams; rq.tab = ragged ? c->dtable : nullptr; rq.pos = &rep;
  const ForwardPlan plan = plan_forward(e, rq, call.ws);
  int rc = run_plan(e, plan, call.ws, on);
  if (rc == SF_OK && pooler && !plan.head_rows)      // the F-row tail left pooler_output in the workspace
    HIP_TRY(sf_launch_copy2(nullptr, nullptr, 0, call.ws.pool_stage, nullptr, (size_t)plan.F * e->D, on, c->dparams));
  return rc;
}

// The graph of `key`, valid for this workspace and position table: the cached one, or a capture of run(cap_stream).
template <typename Run>
static int stream_graph(sf_cache* c, const sf_cache::GraphKey& key, void* workspace, const float* pos_dev, Run&& run, hipGraphExec_t* exec) {
  sf_cache::GraphEntry& g = c->graphs[key];
  if (g.exec && (g.ws != workspace || g.pos != pos_dev)) {      // its nodes carry addresses of another workspace
    (void)hipGraphExecDestroy(g.exec);
    g.exec = nullptr;
  }
  if (!g.exec) {
    hipGraph_t graph = nullptr;
    if (!c->cap_stream) HIP_TRY(hipStreamCreateWithFlags(&c->cap_stream, hipStreamNonBlocking));
    HIP_TRY(hipStreamBeginCapture(c->cap_stream, hipStreamCaptureModeThreadLocal));
    const int rc = run(c->cap_stream);
    const hipError_t ce = hipStreamEndCapture(c->cap_stream, &graph);
    hipError_t ie = hipSuccess;
    if (rc == SF_OK && ce == hipSuccess && graph) ie = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
    if (graph) (void)hipGraphDestroy(graph);
    if (!g.exec) {
      c->graphs.erase(key);
      if (rc != SF_OK) return rc;
      if (ie != hipSuccess) return sf_set_err(SF_ERR_HIP, "hipGraphInstantiate: %s", hipGetErrorString(ie));
      return sf_set_err(SF_ERR_HIP, "stream capture failed: %s", hipGetErrorString(ce));
    }
    g.ws = workspace; g.pos = pos_dev;
  }
  *exec = g.exec;
  return SF_OK;
}

// slab < 0: every stream of the cache advances T_new frames from the one position they share (the lockstep call).
// slab >= 0: that stream alone, as a B = 1 call on its slab of every layer's cache (the prefill of a stream that joins a ragged cache);
// always eager — a prefill happens once per stream, and its position-keyed graph would be captured for a single replay.
static int forward_stream_impl(sf_encoder* e, sf_cache* c, const void* pixels, int pixel_dtype, int T_new,
                               float* last_hidden, float* pooler, float* hidden_states, float* attentions, const float* pos_dev,
                               void* workspace, size_t workspace_bytes, sf_stream stream, int slab = -1) {
  int rc = check_cache_owner(e, c);
  if (rc) return rc;
  const int len = slab < 0 ? c->len() : c->lens[slab];
  StreamCall call;
  StreamPos pos;
  if ((rc = open_stream_call(e, c, slab < 0 ? c->B : 1, T_new, slab < 0, pixels, pixel_dtype, last_hidden, pos_dev, workspace, workspace_bytes, stream,
                             [&]() { return stream_position(c, len, T_new, -1, &pos); }, &call))) return rc;
  const Workspace& ws = call.ws;
  ForwardRequest& rq = call.rq;
  hipStream_t s = call.s;
  rq.pos = &pos;
  std::vector<void*> slab_qkv;
  if (slab >= 0) {
    const size_t per = (size_t)c->cap * c->N * 3 * e->D * (e->compute == SF_COMPUTE_BF16X3 ? 4 : 2);
    for (void* q : c->qkv) slab_qkv.push_back((char*)q + (size_t)slab * per);
    rq.layer_tqkv = slab_qkv.data();
  }
  auto eager = [&]() -> int {
    ForwardRequest q = rq;
    q.last_hidden = last_hidden; q.pooler = pooler; q.hidden_states = hidden_states; q.attentions = attentions;
    const int r = run_forward(e, q, ws, s);
    if (r == SF_OK) { if (slab < 0) c->advance(T_new); else c->lens[slab] += T_new; }
    return r;
  };
  // ---- graph replay (the per-frame sequence is ~100 dependent launches of a few microseconds) -----------------
  // Not when the caller wants the per-layer hidden states (memcpy nodes to caller memory), is capturing the stream
  // itself, or asked for eager launches.
  if (slab >= 0 || !call.graph_ok || hidden_states || attentions) return eager();
  // One new frame per call (the streaming step proper): ONE graph per cache serves every position.  The caller's tensors
  // and the position reach the kernels through a small device block that the patch extraction writes in front of the replay;
  // only the key-pass class is compiled in.
  // Several frames per call keep one graph per (position, count): their attention kernels take the position by value.
  const bool posfree = T_new == 1 && !sf_sw(SW_STREAM_GRAPH_PER_POSITION);
  if (!posfree && T_new == 1 && c->policy == 1) return sf_set_err(SF_ERR_STATE, "SF_STREAM_GRAPH_PER_POSITION cannot serve a sliding-window cache");
  if (!c->warmed.count(kLockstepWarm)) {      // first graph-eligible call of this cache
    rc = eager();
    if (rc == SF_OK) c->warmed.insert(kLockstepWarm);
    return rc;
  }
  const int F = c->B * T_new, kcls = key_pass_class(pos.tk);
  sf_cache::GraphKey key;
  key.kind = posfree ? sf_cache::POSITION_FREE : sf_cache::PER_POSITION; key.rows = c->B; key.T_new = T_new; key.at = posfree ? kcls : len;
  key.pooler = pooler != nullptr; key.pixel_kind = posfree ? call.pk : 0;      // (per position: the patch extraction stays outside the graph)
  // patch extraction reads the caller's frames: outside the graphs.  For the position-free graph the same launch stores the call's
  // parameter block {pixels, outputs, position} that the graph's kernels read, after the graph is there
  SfStreamParams v;
  v.pixels = pixels; v.lhs = last_hidden; v.pooler = pooler; v.t_row = pos.t_row; v.slot = pos.slot; v.tk = pos.tk;
  auto patchify = [&](bool deliver) {
    return sf_launch_patchify(pixels, call.pk, ws.xn_hi, ws.xn_lo, F, e->cfg.num_channels, c->H, c->W, e->cfg.patch_size, s, &e->pixel_norm, nullptr,
                              deliver ? c->dparams : nullptr, deliver ? &v : nullptr, e->Kp);
  };
  if (!posfree) HIP_TRY(patchify(false));
  hipGraphExec_t exec = nullptr;
  rc = stream_graph(c, key, workspace, pos_dev, [&](hipStream_t on) -> int {
    if (posfree) return run_position_free(e, c, call, kcls, false, pooler != nullptr, on);
    ForwardRequest q = rq;      // at this position, into graph-owned outputs
    q.last_hidden = ws.lhs_stage; q.pooler = pooler ? ws.pool_stage : nullptr; q.ready = 1;
    return run_forward(e, q, ws, on);
  }, &exec);
  if (rc) return rc;
  if (posfree) HIP_TRY(patchify(true));
  // (Launching the embedding + first layers eagerly to cover the replay's host-side submit time measured no gain: 0.78 vs 0.77 ms.)
  HIP_TRY(hipGraphLaunch(exec, s));
  if (!posfree)
    HIP_TRY(sf_launch_copy2(ws.lhs_stage, last_hidden, (size_t)F * c->N * e->D, pooler ? ws.pool_stage : nullptr, pooler, (size_t)F * e->D, s));
  c->advance(T_new);
  return SF_OK;
}

extern "C" int sf_forward_stream(sf_encoder* e, sf_cache* c, const void* pixels, int pixel_dtype, int T_new,
                                 float* last_hidden, float* pooler, float* hidden_states, const float* pos_dev, void* workspace,
                                 size_t workspace_bytes, sf_stream stream) {
  return forward_stream_impl(e, c, pixels, pixel_dtype, T_new, last_hidden, pooler, hidden_states, nullptr, pos_dev, workspace, workspace_bytes,
                             stream);
}
// output_attentions while streaming (timesformer_encoder.py:494, 557, 633, 659, 720-754): the spatial attention probabilities of
// the NEW frames, [L, B * T_new, heads, N, N] fp32, as sf_forward_attentions returns them for whole clips
extern "C" int sf_forward_stream_attentions(sf_encoder* e, sf_cache* c, const void* pixels, int pixel_dtype, int T_new,
                                            float* last_hidden, float* pooler, float* hidden_states, float* attentions,
                                            const float* pos_dev, void* workspace, size_t workspace_bytes, sf_stream stream) {
  if (!attentions) return sf_set_err(SF_ERR_INVALID, "null attentions buffer");
  return forward_stream_impl(e, c, pixels, pixel_dtype, T_new, last_hidden, pooler, hidden_states, attentions, pos_dev, workspace,
                             workspace_bytes, stream);
}

// Ragged streaming: the named streams of one batched cache advance, each from its own position.  One frame per stream (the streaming
// step proper): the same launch sequence as the lockstep call of n_streams rows, with {slab, time row, slot, keys} of every row group
// read from a device table that the patch extraction writes next to the parameter block — so one captured graph per (rows, key-pass
// class, pooler, pixel kind) serves every combination of positions.  The key-pass class comes from the longest stream of the call;
// shorter ones are masked by the kernels' own key < tk test.
extern "C" int sf_forward_stream_slots(sf_encoder* e, sf_cache* c, const void* pixels, int pixel_dtype, int T_new, const int* streams,
                                       int n_streams, float* last_hidden, float* pooler, const float* pos_dev, void* workspace,
                                       size_t workspace_bytes, sf_stream stream) {
  int rc = check_cache_owner(e, c);
  if (rc) return rc;
  if (!streams || n_streams <= 0) return sf_set_err(SF_ERR_INVALID, "name at least one stream");
  if (T_new <= 0) return sf_set_err(SF_ERR_INVALID, "T_new must be positive");
  {
    std::vector<char> named(c->B, 0);
    for (int i = 0; i < n_streams; ++i) {
      const int st = streams[i];
      if (st < 0 || st >= c->B) return sf_set_err(SF_ERR_INVALID, "stream %d outside this cache's %d streams (ids are 0 .. %d)", st, c->B, c->B - 1);
      if (named[st]) return sf_set_err(SF_ERR_INVALID, "stream %d named twice: a stream advances once per call, pass several frames of one stream as T_new > 1", st);
      named[st] = 1;
    }
  }
  if (T_new > 1) {
    if (n_streams != 1)
      return sf_set_err(SF_ERR_INVALID, "T_new = %d with %d streams: several frames per call are the prefill of ONE stream — call once per stream with "
                     "n_streams = 1, then advance the streams together one frame per call", T_new, n_streams);
    return forward_stream_impl(e, c, pixels, pixel_dtype, T_new, last_hidden, pooler, nullptr, nullptr, pos_dev, workspace, workspace_bytes, stream,
                               streams[0]);
  }
  if (n_streams > SF_MAX_CALL_STREAMS)
    return sf_set_err(SF_ERR_INVALID, "%d streams in one call; the stream table holds %d: split the call", n_streams, SF_MAX_CALL_STREAMS);
  const int n = n_streams;
  // every stream's position, checked before anything is launched
  SfStreamTable tv;
  memset(&tv, 0, sizeof(tv));
  tv.n = n;
  int max_tk = 0;
  auto positions = [&]() -> int {
    for (int i = 0; i < n; ++i) {
      StreamPos p;
      if (int r = stream_position(c, c->lens[streams[i]], 1, streams[i], &p)) return r;
      tv.e[i] = {streams[i], p.t_row, p.slot, p.tk};
      max_tk = p.tk > max_tk ? p.tk : max_tk;
    }
    return SF_OK;
  };
  StreamCall call;
  if ((rc = open_stream_call(e, c, n, 1, false, pixels, pixel_dtype, last_hidden, pos_dev, workspace, workspace_bytes, stream, positions, &call))) return rc;
  const int kcls = key_pass_class(max_tk);
  sf_cache::GraphKey key;
  key.kind = sf_cache::RAGGED; key.rows = n; key.T_new = 1; key.at = kcls; key.pooler = pooler != nullptr; key.pixel_kind = call.pk;
  // the launch that extracts the patch matrix delivers the parameter block and the table
  const Workspace& ws = call.ws;
  hipStream_t s = call.s;
  SfStreamParams v;
  v.pixels = pixels; v.lhs = last_hidden; v.pooler = pooler; v.t_row = tv.e[0].t_row; v.slot = tv.e[0].slot; v.tk = max_tk;
  auto deliver = [&]() -> hipError_t {
    return sf_launch_patchify(pixels, call.pk, ws.xn_hi, ws.xn_lo, n, e->cfg.num_channels, c->H, c->W, e->cfg.patch_size, s, &e->pixel_norm, nullptr,
                              c->dparams, &v, e->Kp, c->dtable, &tv);
  };
  auto run = [&](hipStream_t on) -> int { return run_position_free(e, c, call, kcls, true, pooler != nullptr, on); };
  if (call.graph_ok && c->warmed.count(key)) {
    hipGraphExec_t exec = nullptr;
    if ((rc = stream_graph(c, key, workspace, pos_dev, run, &exec))) return rc;
    HIP_TRY(deliver());
    HIP_TRY(hipGraphLaunch(exec, s));
  } else {      // graphs off, or the first call of this key
    HIP_TRY(deliver());
    if ((rc = run(s))) return rc;
    if (call.graph_ok) c->warmed.insert(key);
  }
  for (int i = 0; i < n; ++i) c->lens[streams[i]] += 1;
  return SF_OK;
}
