// vocab_train.cpp -- DBoW2::TemplatedVocabulary::create on the device (D/include/DBoW2/TemplatedVocabulary.h:556-994): the host side.
// The host keeps the node table and nothing else: per level it lays out the segments (nodes) and their chunks, starts the narrow form
// for the segments one workgroup can hold and drives the wide form for the others -- k - 1 seeding steps, then rounds, reading one
// control word per round -- and reads back the level's centres and group sizes.  Descriptors, the permutation, associations and the
// per-feature leaf stay in device memory.  At the end the table is renumbered into the reference's creation order (a node's children
// get consecutive ids when the node is processed, nodes are processed depth first), Ni comes from the descent kernel of
// vocab_kernels.hip over the finished tree, and log() runs here, with the host's libm.
#include <math.h>
#include <string.h>

#include <chrono>
#include <vector>

#include "host_internal.h"
#include "vocab_train_internal.h"

static_assert(sizeof(VtSegment) == 40 && sizeof(VtSegState) == 120 && sizeof(VtChunk) == 16, "records shared with the kernels");

namespace {

struct LevelReport { double ms; int32_t rounds, wide, narrow, trivial; };
thread_local LevelReport g_report[VT_MAX_L];
thread_local int g_report_levels = 0;

int effective_wide_min(const orbfe_vocab_train_config& c) {
  return c.wide_min <= 0 ? VT_CHUNK + 1 : std::min(c.wide_min, VT_CHUNK + 1);
}

struct Regions {
  size_t desc, perm, perm_next, assoc, min_dist, leaf_slot, seg, st, centre, count, chunk, chunk_sum, chunk_hist, control, narrow, wide_seg, wide_chunk, word,
      node, wt, image_start, ni, bitmaps, leaf_node, total;
  size_t max_seg, max_chunks, max_wide;
};

Regions regions(const orbfe_vocab_train_config& c, size_t n, size_t n_images) {
  Regions r;
  Layout L;
  r.max_seg = std::max<size_t>(1, n / 2);                       // a node that is clustered holds at least two features (the root: one)
  r.max_chunks = r.max_seg + n / VT_CHUNK + 1;
  r.max_wide = n / (size_t)std::max(effective_wide_min(c), c.k + 1) + 1;
  r.desc = L.add(n * 32);
  r.perm = L.add(n * 4); r.perm_next = L.add(n * 4); r.assoc = L.add(n * 4); r.min_dist = L.add(n * 4); r.leaf_slot = L.add(n * 4);
  r.seg = L.add(r.max_seg * sizeof(VtSegment));
  r.st = L.add(r.max_seg * sizeof(VtSegState));
  r.centre = L.add((n + 1) * 32);                               // sum over a level of min(n_s, k) <= n
  r.count = L.add(r.max_wide * c.k * 256 * 4);
  r.chunk = L.add(r.max_chunks * sizeof(VtChunk));
  r.chunk_sum = L.add(r.max_chunks * 8);
  r.chunk_hist = L.add(r.max_chunks * c.k * 4);
  r.control = L.add(256);
  r.narrow = L.add(r.max_seg * 4);
  r.wide_seg = L.add(r.max_wide * 4);
  r.wide_chunk = L.add((r.max_wide + n / VT_CHUNK + 1) * 4);   // a wide segment's chunks: ceil(n_s / VT_CHUNK) <= 1 + n_s / VT_CHUNK
  r.word = L.add(n * 4); r.node = L.add(n * 4); r.wt = L.add(n * 8);
  r.image_start = L.add((n_images + 1) * 4);
  r.ni = L.add(n * (size_t)c.L * 4);                            // n_words <= L * n: an empty cluster stays a node, so words may outnumber features
  r.bitmaps = L.add(vt_ni_bitmap_words(n) * 4);                 // as many bitmaps of n_words bits as fit (vt_ni_groups)
  r.leaf_node = L.add(n * 4);
  r.total = L.off;
  return r;
}

int validate(const orbfe_vocab_train_config* c, long long n_desc, long long n_images) {
  if (!c) { orbfe_set_error("vocabulary training: null configuration"); return ORBFE_ERR_INVALID; }
  if (c->k < 2 || c->k > VT_MAX_K || c->L < 1 || c->L > VT_MAX_L) {
    orbfe_set_error("vocabulary training: k = %d, L = %d outside 2..20, 1..10", c->k, c->L);
    return ORBFE_ERR_INVALID;
  }
  if (c->scoring < 0 || c->scoring > 5 || c->weighting < 0 || c->weighting > 3) {
    orbfe_set_error("vocabulary training: scoring = %d, weighting = %d outside 0..5, 0..3", c->scoring, c->weighting);
    return ORBFE_ERR_INVALID;
  }
  if (c->max_iterations < 0) { orbfe_set_error("vocabulary training: max_iterations < 0"); return ORBFE_ERR_INVALID; }
  if (n_desc < 1 || n_desc > (1ll << 30)) {
    orbfe_set_error("vocabulary training: %lld descriptors outside 1..2^30", n_desc);
    return ORBFE_ERR_INVALID;
  }
  if (n_images < 1) { orbfe_set_error("vocabulary training: no image"); return ORBFE_ERR_INVALID; }
  return ORBFE_OK;
}

struct HostNode {
  int32_t parent, depth, first_child, n_children;
  uint8_t desc[32];
};
struct Pending { int32_t node, start, n; uint64_t path; };   // a node whose features are clustered at the next level

struct DeviceGuard {   // the calling thread's current device, put back on every way out
  int previous = -1;
  DeviceGuard() { if (hipGetDevice(&previous) != hipSuccess) previous = -1; }
  ~DeviceGuard() { if (previous >= 0) (void)hipSetDevice(previous); }
};

struct Scope {   // what a call owns besides the workspace
  hipStream_t own_stream = nullptr;
  void* d_map = nullptr;
  orbfe_vocabulary* tmp = nullptr;
  ~Scope() {
    if (tmp) orbfe_vocabulary_destroy(tmp);
    if (d_map) (void)hipFree(d_map);
    if (own_stream) (void)hipStreamDestroy(own_stream);
  }
};

// d_ws holds the dense descriptors at regions().desc already
int train(const orbfe_vocab_train_config& cfg, const Regions& R, uint8_t* d_ws, const int32_t* image_start, int n_images, int n,
          int device, int32_t* d_leaf_node, hipStream_t stream, orbfe_vocab_train_stats* stats, orbfe_vocabulary** out) {
  const int k = cfg.k, L = cfg.L, wide_min = effective_wide_min(cfg);
  const int max_it = cfg.max_iterations > 0 ? cfg.max_iterations : ORBFE_VOCAB_TRAIN_MAX_ITERATIONS;
  Scope scope;
  if (!stream) {
    HIPCHK(hipStreamCreateWithFlags(&scope.own_stream, hipStreamNonBlocking));
    stream = scope.own_stream;
  }
  orbfe_vocab_train_stats S;
  memset(&S, 0, sizeof(S));
  VtLevel lv;
  memset(&lv, 0, sizeof(lv));
  lv.desc = d_ws + R.desc;
  lv.perm = (int32_t*)(d_ws + R.perm); lv.perm_next = (int32_t*)(d_ws + R.perm_next);
  lv.assoc = (int32_t*)(d_ws + R.assoc); lv.min_dist = (int32_t*)(d_ws + R.min_dist); lv.leaf_slot = (int32_t*)(d_ws + R.leaf_slot);
  lv.seg = (const VtSegment*)(d_ws + R.seg); lv.st = (VtSegState*)(d_ws + R.st);
  lv.centre = d_ws + R.centre; lv.count = (uint32_t*)(d_ws + R.count);
  lv.chunk = (const VtChunk*)(d_ws + R.chunk); lv.chunk_sum = (int64_t*)(d_ws + R.chunk_sum);
  lv.chunk_hist = (int32_t*)(d_ws + R.chunk_hist); lv.control = (int32_t*)(d_ws + R.control);
  lv.wide_seg = (const int32_t*)(d_ws + R.wide_seg); lv.wide_chunk = (const int32_t*)(d_ws + R.wide_chunk);
  lv.k = k; lv.max_iterations = max_it; lv.seed = cfg.seed;
  int32_t* d_narrow = (int32_t*)(d_ws + R.narrow);
  vt_launch_init(lv.perm, lv.leaf_slot, n, stream);

  std::vector<HostNode> nodes(1);
  nodes[0] = HostNode{0, 0, -1, 0, {0}};
  std::vector<int32_t> slot_node(1, 0);   // slot -> node of the level-order table; slot 0 is the root
  std::vector<Pending> pending(1, Pending{0, 0, n, 0}), next;
  std::vector<VtSegment> seg;
  std::vector<VtChunk> chunk;
  std::vector<VtSegState> st;
  std::vector<int32_t> narrow, wide_seg, wide_chunk;
  std::vector<uint8_t> centre;
  S.nodes_per_level[0] = 1;
  g_report_levels = 0;
  for (int level = 1; level <= L && !pending.empty(); level++) {
    const auto t0 = std::chrono::steady_clock::now();
    seg.clear(); chunk.clear(); narrow.clear(); wide_seg.clear(); wide_chunk.clear();
    int centres = 0, n_wide = 0, n_trivial = 0;
    for (const Pending& p : pending) {
      VtSegment s;
      memset(&s, 0, sizeof(s));
      s.start = p.start; s.n = p.n; s.path = p.path;
      s.kind = p.n <= k ? VT_SEG_TRIVIAL : VT_SEG_KMEANS;
      s.wide = s.kind == VT_SEG_KMEANS && p.n >= wide_min;
      s.chunk0 = (int32_t)chunk.size();
      s.wide_idx = s.wide ? n_wide++ : 0;
      s.centre0 = centres;
      centres += std::min(p.n, k);
      if (s.kind == VT_SEG_TRIVIAL) n_trivial++;
      else if (!s.wide) narrow.push_back((int32_t)seg.size());
      if (s.wide) wide_seg.push_back((int32_t)seg.size());
      for (int off = 0; off < p.n; off += VT_CHUNK) {
        if (s.wide) wide_chunk.push_back((int32_t)chunk.size());
        chunk.push_back(VtChunk{(int32_t)seg.size(), p.start + off, std::min(VT_CHUNK, p.n - off), 0});
      }
      seg.push_back(s);
    }
    if (seg.size() > R.max_seg || chunk.size() > R.max_chunks || (size_t)n_wide > R.max_wide || centres > n ||
        slot_node.size() + (size_t)centres > (size_t)INT32_MAX) {
      orbfe_set_error("vocabulary training: level %d exceeds the workspace layout", level);
      return ORBFE_ERR_CAPACITY;
    }
    lv.n_seg = (int32_t)seg.size(); lv.n_chunks = (int32_t)chunk.size(); lv.level = level;
    lv.n_wide = n_wide; lv.n_wide_chunks = (int32_t)wide_chunk.size();
    lv.slot_base = (int32_t)slot_node.size();
    HIPCHK(hipMemcpyAsync(d_ws + R.seg, seg.data(), seg.size() * sizeof(VtSegment), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_ws + R.chunk, chunk.data(), chunk.size() * sizeof(VtChunk), hipMemcpyHostToDevice, stream));
    if (!narrow.empty()) HIPCHK(hipMemcpyAsync(d_narrow, narrow.data(), narrow.size() * 4, hipMemcpyHostToDevice, stream));
    if (n_wide > 0) {
      HIPCHK(hipMemcpyAsync(d_ws + R.wide_seg, wide_seg.data(), wide_seg.size() * 4, hipMemcpyHostToDevice, stream));
      HIPCHK(hipMemcpyAsync(d_ws + R.wide_chunk, wide_chunk.data(), wide_chunk.size() * 4, hipMemcpyHostToDevice, stream));
    }
    HIPCHK(hipStreamSynchronize(stream));   // the vectors are reused by the next level
    vt_launch_level_begin(lv, stream);
    vt_launch_narrow(lv, d_narrow, (int)narrow.size(), stream);
    int level_rounds = 0;
    if (n_wide > 0) {
      vt_launch_seed_first(lv, stream);
      for (int j = 1; j < k; j++) vt_launch_seed_step(lv, j, stream);
      for (;;) {   // every segment stops by max_it rounds
        int32_t running = 0;
        HIPCHK(hipMemsetAsync(lv.control, 0, 4, stream));
        vt_launch_round(lv, stream);
        HIPCHK(hipMemcpyAsync(&running, lv.control, 4, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        level_rounds++;
        if (running == 0 || level_rounds > max_it) break;
      }
    }
    vt_launch_partition(lv, stream);
    st.resize(seg.size());
    centre.resize((size_t)centres * 32);
    HIPCHK(hipMemcpyAsync(st.data(), lv.st, seg.size() * sizeof(VtSegState), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(centre.data(), lv.centre, centre.size(), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    HIPCHK(hipGetLastError());
    std::swap(lv.perm, lv.perm_next);
    // ---- the level's nodes
    slot_node.resize(slot_node.size() + (size_t)centres, -1);
    next.clear();
    for (size_t s = 0; s < seg.size(); s++) {
      const VtSegState& t = st[s];
      if (t.n_centres < 1 || t.n_centres > std::min(seg[s].n, k) || t.state == VT_RUNNING) {
        orbfe_set_error("vocabulary training: level %d segment %zu came back unfinished", level, s);
        return ORBFE_ERR_HIP;
      }
      if (seg[s].kind == VT_SEG_KMEANS) {
        S.n_kmeans_nodes++;
        S.n_short_seedings += t.short_seeding != 0;
        S.n_empty_clusters += t.empty_events;
        S.n_capped_nodes += t.state == VT_CAPPED;
        S.max_rounds = std::max(S.max_rounds, t.rounds);
        level_rounds = std::max(level_rounds, t.rounds);
      } else {
        S.n_trivial_nodes++;
      }
      HostNode& parent = nodes[pending[s].node];
      parent.first_child = (int32_t)nodes.size();
      parent.n_children = t.n_centres;
      const int depth = parent.depth + 1;
      int start = seg[s].start;
      for (int c = 0; c < t.n_centres; c++) {
        HostNode nd{pending[s].node, depth, -1, 0, {0}};
        memcpy(nd.desc, centre.data() + ((size_t)seg[s].centre0 + c) * 32, 32);
        slot_node[(size_t)lv.slot_base + seg[s].centre0 + c] = (int32_t)nodes.size();
        if (level < L && t.size[c] > 1) next.push_back(Pending{(int32_t)nodes.size(), start, t.size[c], seg[s].path * (uint64_t)k + (uint64_t)c});
        start += t.size[c];
        nodes.push_back(nd);
      }
      S.nodes_per_level[depth] += t.n_centres;
    }
    pending.swap(next);
    if (g_report_levels < VT_MAX_L)
      g_report[g_report_levels++] = LevelReport{std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(),
                                                level_rounds, n_wide, (int32_t)narrow.size(), n_trivial};
  }
  // ---- creation order: children consecutive when the node is processed, subtrees depth first (:784-815)
  const int n_nodes = (int)nodes.size();
  std::vector<int32_t> id(nodes.size(), -1), stack;
  int32_t next_id = 1;
  id[0] = 0;
  stack.push_back(0);
  while (!stack.empty()) {
    const int32_t h = stack.back();
    stack.pop_back();
    const HostNode& nd = nodes[h];
    for (int c = 0; c < nd.n_children; c++) id[nd.first_child + c] = next_id++;
    for (int c = nd.n_children - 1; c >= 0; c--)
      if (nodes[nd.first_child + c].n_children > 0) stack.push_back(nd.first_child + c);
  }
  std::vector<int32_t> parent((size_t)n_nodes, 0);
  std::vector<uint8_t> leaf((size_t)n_nodes, 0), desc((size_t)n_nodes * 32, 0);
  std::vector<double> weight((size_t)n_nodes, 0.0);
  for (int h = 1; h < n_nodes; h++) {
    parent[id[h]] = id[nodes[h].parent];
    leaf[id[h]] = nodes[h].n_children == 0;
    memcpy(&desc[(size_t)id[h] * 32], nodes[h].desc, 32);
  }
  std::vector<int32_t> word_node;
  for (int i = 1; i < n_nodes; i++)
    if (leaf[i]) word_node.push_back(i);
  const int n_words = (int)word_node.size();
  S.n_nodes = n_nodes; S.n_words = n_words;
  if ((size_t)n_words > (size_t)n * (size_t)L) {   // cannot happen: a level creates at most n nodes
    orbfe_set_error("vocabulary training: %d words from %d descriptors exceed the workspace layout", n_words, n);
    return ORBFE_ERR_CAPACITY;
  }
  // ---- setNodeWeights (:941-994)
  if (cfg.weighting == 1 || cfg.weighting == 3) {   // TF, BINARY
    for (int w = 0; w < n_words; w++) weight[word_node[w]] = 1.0;
  } else {
    int rc = orbfe_vocabulary_create(k, L, cfg.scoring, cfg.weighting, n_nodes, parent.data(), leaf.data(), desc.data(), weight.data(), device,
                                     &scope.tmp);
    if (rc != ORBFE_OK) return rc;
    int32_t* d_word = (int32_t*)(d_ws + R.word);
    for (int b = 0; b < n; b += 1 << 24) {
      rc = orbfe_bow_transform_device(scope.tmp, lv.desc + (size_t)b * 32, std::min(1 << 24, n - b), 0, d_word + b,
                                      (int32_t*)(d_ws + R.node) + b, (double*)(d_ws + R.wt) + b, stream);
      if (rc != ORBFE_OK) return rc;
    }
    int32_t* d_ni = (int32_t*)(d_ws + R.ni);
    HIPCHK(hipMemcpyAsync(d_ws + R.image_start, image_start, ((size_t)n_images + 1) * 4, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemsetAsync(d_ni, 0, (size_t)n_words * 4, stream));
    const int groups = vt_ni_groups((size_t)n, (size_t)n_words);
    HIPCHK(hipMemsetAsync(d_ws + R.bitmaps, 0, (size_t)groups * ((n_words + 31) / 32) * 4, stream));
    vt_launch_ni(d_word, (const int32_t*)(d_ws + R.image_start), n_images, n_words, groups, (uint32_t*)(d_ws + R.bitmaps), d_ni, stream);
    std::vector<int32_t> ni((size_t)n_words);
    HIPCHK(hipMemcpyAsync(ni.data(), d_ni, (size_t)n_words * 4, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    HIPCHK(hipGetLastError());
    for (int w = 0; w < n_words; w++)
      if (ni[w] > 0) weight[word_node[w]] = log((double)n_images / (double)ni[w]);
    orbfe_vocabulary_destroy(scope.tmp);
    scope.tmp = nullptr;
  }
  if (d_leaf_node) {
    for (int32_t& v : slot_node) v = v >= 0 ? id[v] : -1;
    HIPCHK(hipMalloc(&scope.d_map, slot_node.size() * 4));
    HIPCHK(hipMemcpyAsync(scope.d_map, slot_node.data(), slot_node.size() * 4, hipMemcpyHostToDevice, stream));
    vt_launch_leaf_translate(lv.leaf_slot, (const int32_t*)scope.d_map, n, d_leaf_node, stream);
    HIPCHK(hipStreamSynchronize(stream));
    HIPCHK(hipGetLastError());
  }
  if (stats) *stats = S;
  return orbfe_vocabulary_create(k, L, cfg.scoring, cfg.weighting, n_nodes, parent.data(), leaf.data(), desc.data(), weight.data(), device, out);
}

int pick_device(int* device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return ORBFE_ERR_NO_DEVICE;
  if (*device < 0 && hipGetDevice(device) != hipSuccess) *device = 0;
  if (*device >= ndev) { orbfe_set_error("vocabulary training: device %d of %d", *device, ndev); return ORBFE_ERR_INVALID; }
  return ORBFE_OK;
}

}  // namespace

extern "C" uint32_t orbfe_vocabulary_training_draw(uint64_t seed, uint32_t level, uint64_t path, uint32_t j) {
  return vt_draw(seed, level, path, j);
}

extern "C" int orbfe_vocabulary_train_workspace_bytes(const orbfe_vocab_train_config* cfg, int64_t n_desc, int n_images, size_t* bytes) {
  if (!bytes) return ORBFE_ERR_INVALID;
  const int rc = validate(cfg, n_desc, n_images);
  if (rc != ORBFE_OK) return rc;
  *bytes = regions(*cfg, (size_t)n_desc, (size_t)n_images).total;
  return ORBFE_OK;
}

extern "C" int orbfe_vocabulary_train(const orbfe_vocab_train_config* cfg, const uint8_t* desc, const int32_t* image_start, int n_images,
                                      int device, int32_t* leaf_node, orbfe_vocab_train_stats* stats, orbfe_vocabulary** vocabulary) {
  if (vocabulary) *vocabulary = nullptr;
  if (!cfg || !desc || !image_start || !vocabulary) { orbfe_set_error("vocabulary training: null pointer"); return ORBFE_ERR_INVALID; }
  if (n_images < 1) return validate(cfg, 1, n_images);
  for (int i = 0; i < n_images; i++)
    if (image_start[i + 1] < image_start[i] || image_start[0] != 0) {
      orbfe_set_error("vocabulary training: image_start is not monotone from 0 at image %d", i);
      return ORBFE_ERR_INVALID;
    }
  const long long n = image_start[n_images];
  int rc = validate(cfg, n, n_images);
  if (rc != ORBFE_OK) return rc;
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;
  if ((rc = pick_device(&device)) != ORBFE_OK) return rc;
  DeviceGuard guard;
  HIPCHK(hipSetDevice(device));
  const Regions R = regions(*cfg, (size_t)n, (size_t)n_images);
  uint8_t* ws = nullptr;
  HIPCHK(hipMalloc((void**)&ws, R.total));
  rc = hip_status("orbfe_vocabulary_train", hipMemcpy(ws + R.desc, desc, (size_t)n * 32, hipMemcpyHostToDevice));
  if (rc == ORBFE_OK)
    rc = train(*cfg, R, ws, image_start, n_images, (int)n, device, leaf_node ? (int32_t*)(ws + R.leaf_node) : nullptr, nullptr, stats, vocabulary);
  if (rc == ORBFE_OK && leaf_node)
    rc = hip_status("orbfe_vocabulary_train", hipMemcpy(leaf_node, ws + R.leaf_node, (size_t)n * 4, hipMemcpyDeviceToHost));
  (void)hipFree(ws);
  if (rc != ORBFE_OK && *vocabulary) { orbfe_vocabulary_destroy(*vocabulary); *vocabulary = nullptr; }
  return rc;
}

extern "C" int orbfe_vocabulary_train_device(const orbfe_vocab_train_config* cfg, const uint8_t* d_desc, const int32_t* d_n, int n_frames,
                                             int cap, void* d_workspace, size_t workspace_bytes, int32_t* d_leaf_node, void* stream,
                                             orbfe_vocab_train_stats* stats, orbfe_vocabulary** vocabulary) {
  if (vocabulary) *vocabulary = nullptr;
  if (!cfg || !d_desc || !d_n || !d_workspace || !vocabulary) { orbfe_set_error("vocabulary training: null pointer"); return ORBFE_ERR_INVALID; }
  if (cap < 1 || ((uintptr_t)d_desc & 15) || ((uintptr_t)d_workspace & 255)) {
    orbfe_set_error("vocabulary training: cap < 1, descriptors not 16-byte aligned or workspace not 256-byte aligned");
    return ORBFE_ERR_INVALID;
  }
  int rc = validate(cfg, 1, n_frames);
  if (rc != ORBFE_OK) return rc;
  {   // the workspace must hold at least the smallest problem of this shape; the true size is checked once the counts are known
    const Regions least = regions(*cfg, 1, (size_t)n_frames);
    if (workspace_bytes < least.total) {
      orbfe_set_error("vocabulary training: workspace of %zu bytes, at least %zu needed", workspace_bytes, least.total);
      return ORBFE_ERR_INVALID;
    }
  }
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;
  int device = -1;
  if ((rc = pick_device(&device)) != ORBFE_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  std::vector<int32_t> cnt((size_t)n_frames), start((size_t)n_frames + 1, 0);
  HIPCHK(hipMemcpyAsync(cnt.data(), d_n, (size_t)n_frames * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  long long n = 0;
  for (int f = 0; f < n_frames; f++) {
    if (cnt[f] < 0 || cnt[f] > cap) { orbfe_set_error("vocabulary training: frame %d holds %d descriptors of %d", f, cnt[f], cap); return ORBFE_ERR_INVALID; }
    n += cnt[f];
    if (n > (1ll << 30)) break;
    start[f + 1] = (int32_t)n;
  }
  if ((rc = validate(cfg, n, n_frames)) != ORBFE_OK) return rc;
  const Regions R = regions(*cfg, (size_t)n, (size_t)n_frames);
  if (workspace_bytes < R.total) {
    orbfe_set_error("vocabulary training: workspace of %zu bytes, %zu needed for %lld descriptors", workspace_bytes, R.total, n);
    return ORBFE_ERR_INVALID;
  }
  uint8_t* ws = (uint8_t*)d_workspace;
  HIPCHK(hipMemcpyAsync(ws + R.image_start, start.data(), start.size() * 4, hipMemcpyHostToDevice, s));
  vt_launch_compact(d_desc, (const int32_t*)(ws + R.image_start), n_frames, cap, ws + R.desc, s);
  HIPCHK(hipStreamSynchronize(s));
  return train(*cfg, R, ws, start.data(), n_frames, (int)n, device, d_leaf_node, s, stats, vocabulary);
}

// per level of the calling thread's last training call: milliseconds, rounds of the slowest node, segments by form.  n_levels entries.
extern "C" int orbfe_debug_vocabulary_train_levels(int max_levels, double* ms, int32_t* rounds, int32_t* wide_segments,
                                                   int32_t* narrow_segments, int32_t* trivial_segments, int* n_levels) {
  if (!n_levels || max_levels < 0) return ORBFE_ERR_INVALID;
  *n_levels = std::min(max_levels, g_report_levels);
  for (int i = 0; i < *n_levels; i++) {
    if (ms) ms[i] = g_report[i].ms;
    if (rounds) rounds[i] = g_report[i].rounds;
    if (wide_segments) wide_segments[i] = g_report[i].wide;
    if (narrow_segments) narrow_segments[i] = g_report[i].narrow;
    if (trivial_segments) trivial_segments[i] = g_report[i].trivial;
  }
  return ORBFE_OK;
}
