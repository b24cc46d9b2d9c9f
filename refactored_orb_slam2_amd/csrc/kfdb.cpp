// kfdb.cpp -- C ABI of the keyframe database (include/orbfe.h: orbfe_kfdb_*).  The handle owns the entries' vectors in one pooled CSR
// in device memory, a record per slot (slots are handed out in add order and never reused before clear: the slot index IS the add
// sequence number that orders the reference's inverted-file lists), the carried relocalisation score per slot and a row of ten
// neighbour slots.  The host keeps a mirror of the slot records, the id -> slot map and the covisibility rows by keyframe id; the
// neighbour rows are resolved to live slots again before the first query after any add, erase or set_covisibles.
// The entry points validate, stage and launch kfdb_kernels.hip.  No CPU fallback: without a device orbfe_kfdb_create is an error.
#include <math.h>
#include <string.h>

#include <array>
#include <atomic>
#include <new>
#include <unordered_map>
#include <vector>

#include "host_internal.h"
#include "kfdb_internal.h"

struct orbfe_kfdb {
  std::mutex mu;
  int device = 0, n_words = 0;
  hipStream_t stream = nullptr;
  std::vector<KfdbSlot> slots;
  std::unordered_map<int64_t, int> live;
  std::unordered_map<int64_t, std::array<int64_t, KFDB_NEIGHBOURS>> covis;
  bool neigh_dirty = false;
  int64_t pool_used = 0, pool_cap = 0;
  int slot_cap = 0;
  int32_t* d_ids = nullptr;
  double* d_vals = nullptr;
  KfdbSlot* d_slots = nullptr;
  int32_t* d_neigh = nullptr;
  float* d_state = nullptr;
  uint8_t *d_block = nullptr, *h_block = nullptr;
  size_t block_cap = 0;
};

namespace {

std::atomic<int> g_arrangement{0};   // orbfe_debug_kfdb_arrangement

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int device) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    (void)hipSetDevice(device);
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// grows a device array to `want` elements, keeping the first `keep`; new bytes are zero
template <class T>
hipError_t grow(T** p, size_t keep, size_t want) {
  T* q = nullptr;
  hipError_t e = hipMalloc((void**)&q, want * sizeof(T));
  if (e != hipSuccess) return e;
  e = hipMemset(q, 0, want * sizeof(T));
  if (e == hipSuccess && keep) e = hipMemcpy(q, *p, keep * sizeof(T), hipMemcpyDeviceToDevice);
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);   // neither call has to be complete when it returns
  if (e != hipSuccess) {
    (void)hipFree(q);
    return e;
  }
  if (*p) (void)hipFree(*p);
  *p = q;
  return hipSuccess;
}

int ensure_block(orbfe_kfdb* db, size_t bytes) {
  if (bytes <= db->block_cap) return ORBFE_OK;
  const size_t want = bytes + bytes / 2;
  if (db->d_block) (void)hipFree(db->d_block);
  if (db->h_block) (void)hipHostFree(db->h_block);
  db->d_block = db->h_block = nullptr;
  db->block_cap = 0;
  hipError_t e = hipMalloc((void**)&db->d_block, want);
  if (e == hipSuccess) e = hipHostMalloc((void**)&db->h_block, want, hipHostMallocDefault);
  if (e != hipSuccess) return hip_status("kfdb: work space", e);
  db->block_cap = want;
  return ORBFE_OK;
}

// one sparse vector: 0 <= n <= 4096, ids ascend strictly in [0, n_words), values finite and positive
bool vector_ok(const char* where, const int32_t* ids, const double* vals, int n, int n_words) {
  if (n < 0 || n > ORBFE_KFDB_MAX_WORDS) {
    orbfe_set_error("%s: %d words (0 .. %d)", where, n, ORBFE_KFDB_MAX_WORDS);
    return false;
  }
  if (n > 0 && (!ids || !vals)) {
    orbfe_set_error("%s: ids and values are required", where);
    return false;
  }
  for (int i = 0; i < n; i++) {
    if (ids[i] < 0 || ids[i] >= n_words || (i > 0 && ids[i] <= ids[i - 1])) {
      orbfe_set_error("%s: word %d has id %d: ids ascend strictly and lie in [0, %d)", where, i, ids[i], n_words);
      return false;
    }
    if (!(vals[i] > 0.0) || !isfinite(vals[i])) {
      orbfe_set_error("%s: word %d has value %g: values are finite and positive", where, i, vals[i]);
      return false;
    }
  }
  return true;
}

bool queries_ok(const char* where, const orbfe_kfdb* db, int Q, const int32_t* q_off, const int32_t* q_ids, const double* q_vals) {
  if (Q < 0 || Q > ORBFE_KFDB_MAX_QUERIES) {
    orbfe_set_error("%s: Q %d (0 .. %d)", where, Q, ORBFE_KFDB_MAX_QUERIES);
    return false;
  }
  if (Q == 0) return true;
  if (!q_off || q_off[0] != 0) {
    orbfe_set_error("%s: q_offsets are required and start at 0", where);
    return false;
  }
  for (int q = 0; q < Q; q++) {
    const int n = q_off[q + 1] - q_off[q];
    if (n < 0 || n > ORBFE_KFDB_MAX_WORDS) {
      orbfe_set_error("%s: query %d has %d words (0 .. %d)", where, q, n, ORBFE_KFDB_MAX_WORDS);
      return false;
    }
    if (!vector_ok(where, q_ids ? q_ids + q_off[q] : nullptr, q_vals ? q_vals + q_off[q] : nullptr, n, db->n_words)) return false;
  }
  return true;
}

bool loop_ok(int Q, const float* min_score, const int32_t* c_off, const int64_t* c_ids) {
  if (Q == 0) return true;
  if (!min_score || !c_off || c_off[0] != 0) {
    orbfe_set_error("kfdb detect loop: min_score and conn_offsets are required, conn_offsets start at 0");
    return false;
  }
  for (int q = 0; q < Q; q++) {
    if (!isfinite(min_score[q]) || signbit(min_score[q])) {
      orbfe_set_error("kfdb detect loop: min_score[%d] = %g: finite and not negative", q, (double)min_score[q]);
      return false;
    }
    const int n = c_off[q + 1] - c_off[q];
    if (n < 0 || (n > 0 && !c_ids)) {
      orbfe_set_error("kfdb detect loop: query %d has %d connected ids", q, n);
      return false;
    }
    for (int i = 1; i < n; i++)
      if (c_ids[c_off[q] + i] <= c_ids[c_off[q] + i - 1]) {
        orbfe_set_error("kfdb detect loop: the connected ids of query %d must ascend strictly", q);
        return false;
      }
  }
  return true;
}

bool outputs_ok(const char* where, const orbfe_kfdb* db, int Q, int cand_cap, const void* cand, const void* n_cand) {
  if (cand_cap < 0 || (cand_cap > 0 && !cand) || (Q > 0 && !n_cand)) {
    orbfe_set_error("%s: cand_cap %d (>= 0), cand is required with cand_cap > 0, n_cand always", where, cand_cap);
    return false;
  }
  (void)db;
  return true;
}

int cells_ok(const char* where, const orbfe_kfdb* db, int Q, int cand_cap) {
  if ((uint64_t)Q * db->slots.size() > (uint64_t)ORBFE_KFDB_MAX_CELLS || (uint64_t)Q * (uint64_t)cand_cap > (uint64_t)ORBFE_KFDB_MAX_CELLS) {
    orbfe_set_error("%s: Q x slots (%d x %zu) and Q x cand_cap (%d) are limited to %d", where, Q, db->slots.size(), cand_cap, ORBFE_KFDB_MAX_CELLS);
    return ORBFE_ERR_CAPACITY;
  }
  return ORBFE_OK;
}

// the neighbour rows as slots, for the entries that are live now
int resolve_neighbours(orbfe_kfdb* db) {
  if (!db->neigh_dirty) return ORBFE_OK;
  const size_t n = db->slots.size();
  if (n) {
    std::vector<int32_t> rows(n * KFDB_NEIGHBOURS, -1);
    for (size_t s = 0; s < n; s++) {
      if (!db->slots[s].live) continue;
      const auto it = db->covis.find(db->slots[s].id);
      if (it == db->covis.end()) continue;
      for (int k = 0; k < KFDB_NEIGHBOURS; k++) {
        const auto l = db->live.find(it->second[k]);
        if (it->second[k] >= 0 && l != db->live.end()) rows[s * KFDB_NEIGHBOURS + k] = l->second;
      }
    }
    const hipError_t e = hipMemcpy(db->d_neigh, rows.data(), rows.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_status("kfdb: neighbour rows", e);
  }
  db->neigh_dirty = false;
  return ORBFE_OK;
}

void fill_database(const orbfe_kfdb* db, KfdbLaunch& L) {
  L.ids = db->d_ids; L.vals = db->d_vals; L.slots = db->d_slots; L.neigh = db->d_neigh; L.state = db->d_state;
  L.n_slots = (int)db->slots.size();
}

// the work arrays of a detection behind `base` of the device block; returns the end
size_t fill_work(KfdbLaunch& L, uint8_t* d, Layout& Lo, int Q) {
  const size_t cells = (size_t)Q * (size_t)L.n_slots * 4;
  L.words = (int32_t*)(d + Lo.add(cells));
  L.score = (float*)(d + Lo.add(cells));
  L.first = (int32_t*)(d + Lo.add(cells));
  L.carried = (float*)(d + Lo.add(cells));
  for (int k = 0; k < 6; k++) L.sel[k] = (int32_t*)(d + Lo.add(cells));
  L.qstat = (int32_t*)(d + Lo.add((size_t)Q * 12));
  return Lo.off;
}

int detect_host(orbfe_kfdb* db, int loop, int Q, const int32_t* q_off, const int32_t* q_ids, const double* q_vals, const float* min_score,
                const int32_t* c_off, const int64_t* c_ids, int cand_cap, int64_t* cand, int32_t* n_cand, orbfe_kfdb_query_info* info,
                int32_t* common_words, float* scores) {
  const char* where = loop ? "kfdb detect loop" : "kfdb detect relocalization";
  if (!db) {
    orbfe_set_error("%s: null handle", where);
    return ORBFE_ERR_INVALID;
  }
  std::lock_guard<std::mutex> lk(db->mu);
  if (!queries_ok(where, db, Q, q_off, q_ids, q_vals) || !outputs_ok(where, db, Q, cand_cap, cand, n_cand)) return ORBFE_ERR_INVALID;
  if (loop && !loop_ok(Q, min_score, c_off, c_ids)) return ORBFE_ERR_INVALID;
  int rc;
  if ((rc = cells_ok(where, db, Q, cand_cap))) return rc;
  if (Q == 0) return ORBFE_OK;
  DeviceGuard g(db->device);
  if ((rc = resolve_neighbours(db))) return rc;
  const size_t nw = (size_t)q_off[Q], nc = loop ? (size_t)c_off[Q] : 0, n = db->slots.size();
  Layout Lo;
  const size_t o_qoff = Lo.add((size_t)(Q + 1) * 4), o_qids = Lo.add(nw * 4), o_qvals = Lo.add(nw * 8), o_ms = Lo.add((size_t)Q * 4),
               o_coff = Lo.add((size_t)(Q + 1) * 4), o_cids = Lo.add(nc * 8);
  const size_t in_end = Lo.off;
  const size_t o_ncand = Lo.add((size_t)Q * 4), o_info = Lo.add((size_t)Q * sizeof(orbfe_kfdb_query_info)),
               o_cand = Lo.add((size_t)Q * cand_cap * 8);
  KfdbLaunch L;
  memset(&L, 0, sizeof(L));
  fill_database(db, L);
  const size_t o_words = Lo.off;   // fill_work puts words and score first: the optional downloads
  if ((rc = ensure_block(db, o_words + (size_t)KFDB_WORK_ARRAYS * (((size_t)Q * n * 4 + 255) & ~(size_t)255) + (((size_t)Q * 12 + 255) & ~(size_t)255))))
    return rc;
  uint8_t *d = db->d_block, *h = db->h_block;
  fill_work(L, d, Lo, Q);
  const size_t o_score = (uint8_t*)L.score - d, o_first = (uint8_t*)L.first - d;
  const bool dense = common_words || scores;
  const size_t out_end = dense ? o_first : o_words;

  memcpy(h + o_qoff, q_off, (size_t)(Q + 1) * 4);
  if (nw) {
    memcpy(h + o_qids, q_ids, nw * 4);
    memcpy(h + o_qvals, q_vals, nw * 8);
  }
  if (loop) {
    memcpy(h + o_ms, min_score, (size_t)Q * 4);
    memcpy(h + o_coff, c_off, (size_t)(Q + 1) * 4);
    if (nc) memcpy(h + o_cids, c_ids, nc * 8);
  }
  hipStream_t s = db->stream;
  hipError_t e = hipMemcpyAsync(d, h, in_end, hipMemcpyHostToDevice, s);
  if (e != hipSuccess) return hip_status(where, e);
  L.Q = Q; L.loop = loop; L.fused = g_arrangement.load();
  L.q_off = (const int32_t*)(d + o_qoff); L.q_ids = (const int32_t*)(d + o_qids); L.q_vals = (const double*)(d + o_qvals);
  L.min_score = (const float*)(d + o_ms); L.c_off = (const int32_t*)(d + o_coff); L.c_ids = (const int64_t*)(d + o_cids);
  L.cand = (int64_t*)(d + o_cand); L.cand_cap = cand_cap; L.n_cand = (int32_t*)(d + o_ncand); L.info = (orbfe_kfdb_query_info*)(d + o_info);
  orbfe_launch_kfdb_detect(L, s);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(h + o_ncand, d + o_ncand, out_end - o_ncand, hipMemcpyDeviceToHost, s);
  const hipError_t e2 = hipStreamSynchronize(s);   // also on an error: the stream may still read the pinned block
  if (e != hipSuccess || e2 != hipSuccess) return hip_status(where, e != hipSuccess ? e : e2);
  const int32_t* h_n = (const int32_t*)(h + o_ncand);
  const orbfe_kfdb_query_info* h_info = (const orbfe_kfdb_query_info*)(h + o_info);
  memcpy(n_cand, h_n, (size_t)Q * 4);
  if (info) memcpy(info, h_info, (size_t)Q * sizeof(*info));
  for (int q = 0; q < Q; q++) {   // rows behind the counts stay as they are
    const int k = h_n[q] < cand_cap ? h_n[q] : cand_cap;
    if (k > 0) memcpy(cand + (size_t)q * cand_cap, h + o_cand + (size_t)q * cand_cap * 8, (size_t)k * 8);
  }
  if (dense) {
    const int32_t* hw = (const int32_t*)(h + o_words);
    const float* hs = (const float*)(h + o_score);
    for (int q = 0; q < Q; q++)
      for (size_t sl = 0; sl < n; sl++) {
        const size_t o = (size_t)q * n + sl;
        if (hw[o] > h_info[q].min_common_words) {   // scored; everything else is left untouched
          if (common_words) common_words[o] = hw[o];
          if (scores) scores[o] = hs[o];
        }
      }
  }
  return ORBFE_OK;
}

int detect_device(orbfe_kfdb* db, int loop, int Q, const int32_t* q_off, const int32_t* q_ids, const double* q_vals, const float* min_score,
                  const int32_t* c_off, const int64_t* c_ids, int cand_cap, int64_t* cand, int32_t* n_cand, orbfe_kfdb_query_info* info,
                  int32_t* common_words, float* scores, void* stream) {
  const char* where = loop ? "kfdb detect loop (device)" : "kfdb detect relocalization (device)";
  if (!db) {
    orbfe_set_error("%s: null handle", where);
    return ORBFE_ERR_INVALID;
  }
  std::lock_guard<std::mutex> lk(db->mu);
  if (Q < 0 || Q > ORBFE_KFDB_MAX_QUERIES) {
    orbfe_set_error("%s: Q %d (0 .. %d)", where, Q, ORBFE_KFDB_MAX_QUERIES);
    return ORBFE_ERR_INVALID;
  }
  if (Q > 0 && (!q_off || !q_ids || !q_vals || (loop && (!min_score || !c_off || !c_ids)))) {
    orbfe_set_error("%s: the query arrays are required%s", where, loop ? ", min_score and both connected arrays too" : "");
    return ORBFE_ERR_INVALID;
  }
  if (!outputs_ok(where, db, Q, cand_cap, cand, n_cand)) return ORBFE_ERR_INVALID;
  if (((uintptr_t)q_off & 3) || ((uintptr_t)q_ids & 3) || ((uintptr_t)q_vals & 7) || ((uintptr_t)min_score & 3) || ((uintptr_t)c_off & 3) ||
      ((uintptr_t)c_ids & 7) || ((uintptr_t)cand & 7) || ((uintptr_t)n_cand & 3) || ((uintptr_t)info & 3) || ((uintptr_t)common_words & 3) ||
      ((uintptr_t)scores & 3)) {
    orbfe_set_error("%s: 4-byte records must be 4-byte aligned, 8-byte records 8-byte aligned", where);
    return ORBFE_ERR_INVALID;
  }
  int rc;
  if ((rc = cells_ok(where, db, Q, cand_cap))) return rc;
  if (Q == 0) return ORBFE_OK;
  DeviceGuard g(db->device);
  if ((rc = resolve_neighbours(db))) return rc;
  KfdbLaunch L;
  memset(&L, 0, sizeof(L));
  fill_database(db, L);
  const size_t n = db->slots.size();
  if ((rc = ensure_block(db, (size_t)KFDB_WORK_ARRAYS * (((size_t)Q * n * 4 + 255) & ~(size_t)255) + (((size_t)Q * 12 + 255) & ~(size_t)255)))) return rc;
  Layout Lo;
  fill_work(L, db->d_block, Lo, Q);
  L.Q = Q; L.loop = loop; L.fused = g_arrangement.load();
  L.q_off = q_off; L.q_ids = q_ids; L.q_vals = q_vals; L.min_score = min_score; L.c_off = c_off; L.c_ids = c_ids;
  L.cand = cand; L.cand_cap = cand_cap; L.n_cand = n_cand; L.info = info; L.o_words = common_words; L.o_scores = scores;
  orbfe_launch_kfdb_detect(L, (hipStream_t)stream);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_status(where, e);
  return ORBFE_OK;
}

}  // namespace

extern "C" int orbfe_debug_kfdb_arrangement(int arrangement) {
  if (arrangement != 0 && arrangement != 1) {
    orbfe_set_error("kfdb arrangement %d (0: separate score pass, 1: scores in the common pass)", arrangement);
    return ORBFE_ERR_INVALID;
  }
  g_arrangement.store(arrangement);
  return ORBFE_OK;
}

extern "C" int orbfe_kfdb_create(int n_words, int scoring, int device, orbfe_kfdb** out) {
  if (!out) {
    orbfe_set_error("kfdb create: out is required");
    return ORBFE_ERR_INVALID;
  }
  *out = nullptr;
  if (n_words < 1) {
    orbfe_set_error("kfdb create: n_words %d (>= 1)", n_words);
    return ORBFE_ERR_INVALID;
  }
  if (scoring != ORBFE_KFDB_L1_NORM) {
    orbfe_set_error("kfdb create: scoring %d: only ORBFE_KFDB_L1_NORM (ORBvoc's scoring) is implemented", scoring);
    return ORBFE_ERR_INVALID;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
    orbfe_set_error("no HIP device available (liborbfe has no CPU fallback)");
    return ORBFE_ERR_NO_DEVICE;
  }
  if (device >= ndev) {
    orbfe_set_error("kfdb create: device %d of %d", device, ndev);
    return ORBFE_ERR_INVALID;
  }
  if (device < 0 && hipGetDevice(&device) != hipSuccess) device = 0;
  orbfe_kfdb* db = new (std::nothrow) orbfe_kfdb;
  if (!db) return ORBFE_ERR_ALLOC;
  db->device = device;
  db->n_words = n_words;
  DeviceGuard g(device);
  const hipError_t e = hipStreamCreateWithFlags(&db->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    delete db;
    return hip_status("kfdb create: stream", e);
  }
  *out = db;
  return ORBFE_OK;
}

extern "C" int orbfe_kfdb_destroy(orbfe_kfdb* db) {
  if (!db) return ORBFE_OK;
  {
    DeviceGuard g(db->device);
    if (db->stream) {
      (void)hipStreamSynchronize(db->stream);
      (void)hipStreamDestroy(db->stream);
    }
    if (db->d_ids) (void)hipFree(db->d_ids);
    if (db->d_vals) (void)hipFree(db->d_vals);
    if (db->d_slots) (void)hipFree(db->d_slots);
    if (db->d_neigh) (void)hipFree(db->d_neigh);
    if (db->d_state) (void)hipFree(db->d_state);
    if (db->d_block) (void)hipFree(db->d_block);
    if (db->h_block) (void)hipHostFree(db->h_block);
  }
  delete db;
  return ORBFE_OK;
}

extern "C" int orbfe_kfdb_clear(orbfe_kfdb* db) {
  if (!db) {
    orbfe_set_error("kfdb clear: null handle");
    return ORBFE_ERR_INVALID;
  }
  std::lock_guard<std::mutex> lk(db->mu);
  DeviceGuard g(db->device);
  if (db->slot_cap) {   // the carried scores start at 0 again; everything else is rewritten by add
    hipError_t e = hipMemset(db->d_state, 0, (size_t)db->slot_cap * sizeof(float));
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);   // a memset may return before it ran; the queries use other streams
    if (e != hipSuccess) return hip_status("kfdb clear", e);
  }
  db->slots.clear();
  db->live.clear();
  db->covis.clear();
  db->pool_used = 0;
  db->neigh_dirty = false;
  return ORBFE_OK;
}

extern "C" int orbfe_kfdb_size(const orbfe_kfdb* db, int* n_live, int* n_slots) {
  if (!db) {
    orbfe_set_error("kfdb size: null handle");
    return ORBFE_ERR_INVALID;
  }
  std::lock_guard<std::mutex> lk(const_cast<orbfe_kfdb*>(db)->mu);
  if (n_live) *n_live = (int)db->live.size();
  if (n_slots) *n_slots = (int)db->slots.size();
  return ORBFE_OK;
}

extern "C" int orbfe_kfdb_slots(const orbfe_kfdb* db, int64_t* kf_ids, int cap, int* n_slots) {
  if (!db || cap < 0 || (cap > 0 && !kf_ids)) {
    orbfe_set_error("kfdb slots: handle, cap %d (>= 0) and kf_ids with cap > 0 are required", cap);
    return ORBFE_ERR_INVALID;
  }
  std::lock_guard<std::mutex> lk(const_cast<orbfe_kfdb*>(db)->mu);
  const int n = (int)db->slots.size();
  for (int s = 0; s < n && s < cap; s++) kf_ids[s] = db->slots[s].id;
  if (n_slots) *n_slots = n;
  return ORBFE_OK;
}

extern "C" int orbfe_kfdb_add(orbfe_kfdb* db, int64_t kf_id, const int32_t* bow_ids, const double* bow_vals, int n) {
  if (!db) {
    orbfe_set_error("kfdb add: null handle");
    return ORBFE_ERR_INVALID;
  }
  std::lock_guard<std::mutex> lk(db->mu);
  if (kf_id < 0) {
    orbfe_set_error("kfdb add: keyframe id %lld (>= 0)", (long long)kf_id);
    return ORBFE_ERR_INVALID;
  }
  if (!vector_ok("kfdb add", bow_ids, bow_vals, n, db->n_words)) return ORBFE_ERR_INVALID;
  if (db->live.count(kf_id)) {
    orbfe_set_error("kfdb add: keyframe %lld is in the database already (erase it first)", (long long)kf_id);
    return ORBFE_ERR_INVALID;
  }
  if (db->slots.size() >= (size_t)ORBFE_KFDB_MAX_SLOTS) {
    orbfe_set_error("kfdb add: %d slots are in use (erased ones count until clear)", ORBFE_KFDB_MAX_SLOTS);
    return ORBFE_ERR_CAPACITY;
  }
  DeviceGuard g(db->device);
  hipError_t e = hipSuccess;
  const int s = (int)db->slots.size();
  if (s + 1 > db->slot_cap) {
    const int want = db->slot_cap ? db->slot_cap * 2 : 1024;
    e = grow(&db->d_slots, (size_t)s, (size_t)want);
    if (e == hipSuccess) e = grow(&db->d_state, (size_t)s, (size_t)want);
    if (e == hipSuccess) e = grow(&db->d_neigh, (size_t)s * KFDB_NEIGHBOURS, (size_t)want * KFDB_NEIGHBOURS);
    if (e != hipSuccess) return hip_status("kfdb add: growing the slot arrays", e);
    db->slot_cap = want;
    db->neigh_dirty = true;
  }
  if (db->pool_used + n > db->pool_cap) {
    int64_t want = db->pool_cap ? db->pool_cap * 2 : (int64_t)1 << 20;
    while (want < db->pool_used + n) want *= 2;
    e = grow(&db->d_ids, (size_t)db->pool_used, (size_t)want);
    if (e == hipSuccess) e = grow(&db->d_vals, (size_t)db->pool_used, (size_t)want);
    if (e != hipSuccess) return hip_status("kfdb add: growing the pool", e);
    db->pool_cap = want;
  }
  KfdbSlot sl;
  sl.off = db->pool_used; sl.id = kf_id; sl.len = n; sl.live = 1;
  if (n) {
    e = hipMemcpy(db->d_ids + sl.off, bow_ids, (size_t)n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(db->d_vals + sl.off, bow_vals, (size_t)n * 8, hipMemcpyHostToDevice);
  }
  const float zero = 0.0f;   // mRelocScore starts at 0 here (the reference leaves it uninitialised)
  if (e == hipSuccess) e = hipMemcpy(db->d_state + s, &zero, sizeof(zero), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(db->d_slots + s, &sl, sizeof(sl), hipMemcpyHostToDevice);
  if (e != hipSuccess) return hip_status("kfdb add: upload", e);
  db->slots.push_back(sl);
  db->live[kf_id] = s;
  db->pool_used += n;
  db->neigh_dirty = true;
  return ORBFE_OK;
}

extern "C" int orbfe_kfdb_erase(orbfe_kfdb* db, int64_t kf_id) {
  if (!db) {
    orbfe_set_error("kfdb erase: null handle");
    return ORBFE_ERR_INVALID;
  }
  std::lock_guard<std::mutex> lk(db->mu);
  const auto it = db->live.find(kf_id);
  if (it == db->live.end()) return ORBFE_OK;   // as the reference: nothing to remove
  DeviceGuard g(db->device);
  const int s = it->second;
  KfdbSlot sl = db->slots[s];
  sl.id = -1; sl.live = 0;
  const hipError_t e = hipMemcpy(db->d_slots + s, &sl, sizeof(sl), hipMemcpyHostToDevice);
  if (e != hipSuccess) return hip_status("kfdb erase", e);
  db->slots[s] = sl;
  db->live.erase(it);
  db->neigh_dirty = true;
  return ORBFE_OK;
}

extern "C" int orbfe_kfdb_set_covisibles(orbfe_kfdb* db, int n_rows, const int64_t* kf_ids, const int64_t* neigh) {
  if (!db || n_rows < 0 || (n_rows > 0 && (!kf_ids || !neigh))) {
    orbfe_set_error("kfdb set covisibles: handle, n_rows %d (>= 0), kf_ids and neigh are required", n_rows);
    return ORBFE_ERR_INVALID;
  }
  std::lock_guard<std::mutex> lk(db->mu);
  for (int r = 0; r < n_rows; r++)
    if (kf_ids[r] < 0) {
      orbfe_set_error("kfdb set covisibles: row %d has keyframe id %lld (>= 0)", r, (long long)kf_ids[r]);
      return ORBFE_ERR_INVALID;
    }
  for (int r = 0; r < n_rows; r++) {
    std::array<int64_t, KFDB_NEIGHBOURS> row;
    for (int k = 0; k < KFDB_NEIGHBOURS; k++) row[k] = neigh[(size_t)r * KFDB_NEIGHBOURS + k];
    db->covis[kf_ids[r]] = row;
  }
  if (n_rows) db->neigh_dirty = true;
  return ORBFE_OK;
}

extern "C" int orbfe_kfdb_score(orbfe_kfdb* db, const int32_t* q_ids, const double* q_vals, int n, const int64_t* kf_ids, int m, float* out) {
  if (!db) {
    orbfe_set_error("kfdb score: null handle");
    return ORBFE_ERR_INVALID;
  }
  std::lock_guard<std::mutex> lk(db->mu);
  if (!vector_ok("kfdb score", q_ids, q_vals, n, db->n_words)) return ORBFE_ERR_INVALID;
  if (m < 0 || m > ORBFE_KFDB_MAX_SLOTS || (m > 0 && (!kf_ids || !out))) {
    orbfe_set_error("kfdb score: m %d (0 .. %d), kf_ids and out are required", m, ORBFE_KFDB_MAX_SLOTS);
    return ORBFE_ERR_INVALID;
  }
  if (m == 0) return ORBFE_OK;
  DeviceGuard g(db->device);
  Layout Lo;
  const size_t o_qoff = Lo.add(8), o_qids = Lo.add((size_t)n * 4), o_qvals = Lo.add((size_t)n * 8), o_list = Lo.add((size_t)m * 4);
  const size_t in_end = Lo.off;
  const size_t o_out = Lo.add((size_t)m * 4);
  int rc;
  if ((rc = ensure_block(db, Lo.off))) return rc;
  uint8_t *d = db->d_block, *h = db->h_block;
  const int32_t off[2] = {0, n};
  memcpy(h + o_qoff, off, sizeof(off));
  if (n) {
    memcpy(h + o_qids, q_ids, (size_t)n * 4);
    memcpy(h + o_qvals, q_vals, (size_t)n * 8);
  }
  int32_t* list = (int32_t*)(h + o_list);
  for (int k = 0; k < m; k++) {
    const auto it = db->live.find(kf_ids[k]);
    list[k] = it == db->live.end() ? -1 : it->second;
  }
  hipStream_t s = db->stream;
  hipError_t e = hipMemcpyAsync(d, h, in_end, hipMemcpyHostToDevice, s);
  if (e != hipSuccess) return hip_status("kfdb score: upload", e);
  KfdbLaunch L;
  memset(&L, 0, sizeof(L));
  fill_database(db, L);
  L.Q = 1;
  L.q_off = (const int32_t*)(d + o_qoff); L.q_ids = (const int32_t*)(d + o_qids); L.q_vals = (const double*)(d + o_qvals);
  orbfe_launch_kfdb_score_list(L, (const int32_t*)(d + o_list), m, (float*)(d + o_out), s);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(h + o_out, d + o_out, (size_t)m * 4, hipMemcpyDeviceToHost, s);
  const hipError_t e2 = hipStreamSynchronize(s);
  if (e != hipSuccess || e2 != hipSuccess) return hip_status("kfdb score", e != hipSuccess ? e : e2);
  memcpy(out, h + o_out, (size_t)m * 4);
  return ORBFE_OK;
}

extern "C" int orbfe_kfdb_detect_relocalization(orbfe_kfdb* db, int Q, const int32_t* q_offsets, const int32_t* q_ids, const double* q_vals,
                                                int cand_cap, int64_t* cand, int32_t* n_cand, orbfe_kfdb_query_info* info,
                                                int32_t* common_words, float* scores) {
  return detect_host(db, 0, Q, q_offsets, q_ids, q_vals, nullptr, nullptr, nullptr, cand_cap, cand, n_cand, info, common_words, scores);
}

extern "C" int orbfe_kfdb_detect_loop(orbfe_kfdb* db, int Q, const int32_t* q_offsets, const int32_t* q_ids, const double* q_vals,
                                      const float* min_score, const int32_t* conn_offsets, const int64_t* conn_ids, int cand_cap,
                                      int64_t* cand, int32_t* n_cand, orbfe_kfdb_query_info* info, int32_t* common_words, float* scores) {
  return detect_host(db, 1, Q, q_offsets, q_ids, q_vals, min_score, conn_offsets, conn_ids, cand_cap, cand, n_cand, info, common_words,
                     scores);
}

extern "C" int orbfe_kfdb_detect_relocalization_device(orbfe_kfdb* db, int Q, const int32_t* d_q_offsets, const int32_t* d_q_ids,
                                                       const double* d_q_vals, int cand_cap, int64_t* d_cand, int32_t* d_n_cand,
                                                       orbfe_kfdb_query_info* d_info, int32_t* d_common_words, float* d_scores,
                                                       void* stream) {
  return detect_device(db, 0, Q, d_q_offsets, d_q_ids, d_q_vals, nullptr, nullptr, nullptr, cand_cap, d_cand, d_n_cand, d_info,
                       d_common_words, d_scores, stream);
}

extern "C" int orbfe_kfdb_detect_loop_device(orbfe_kfdb* db, int Q, const int32_t* d_q_offsets, const int32_t* d_q_ids,
                                             const double* d_q_vals, const float* d_min_score, const int32_t* d_conn_offsets,
                                             const int64_t* d_conn_ids, int cand_cap, int64_t* d_cand, int32_t* d_n_cand,
                                             orbfe_kfdb_query_info* d_info, int32_t* d_common_words, float* d_scores, void* stream) {
  return detect_device(db, 1, Q, d_q_offsets, d_q_ids, d_q_vals, d_min_score, d_conn_offsets, d_conn_ids, cand_cap, d_cand, d_n_cand,
                       d_info, d_common_words, d_scores, stream);
}
