// api.hip - host side of the C ABI declared in include/hgs_rast.h: buffer carving and the
// launch sequences.  No allocation, no host synchronisation; the only process-wide state is one DeviceState per device
// (CU count, side stream, which kernels had their dynamic-LDS limit raised), each part filled at its first use.
//
// Forward launch chain (one stream, no host round trip), for all B views of a call at once:
//   preprocess_fwd -> tiles -> fill (+ tile order) [status published] -> sort_{huge,large,lds} (+ cell lists,
//   backward work items) -> render_fwd (one workgroup per tile, heavy first)
// Backward: render_bwd (persistent waves, four cell-list segments each) -> pair_reduce -> preprocess_bwd.
#include "hgs_common.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <mutex>

// The forward kernels and the per-Gaussian backward are included here (one translation
// unit, SLP vectorisation on: the forward blend is latency-bound and profits from v_pk_*).
#ifdef HGS_TIMELINE
__device__ unsigned long long hgs_tl[HGS_TL_KERNELS][HGS_TL_SLOTS][4];
#endif
#include "preprocess.hip"
#include "binning.hip"
#include "render_fwd.hip"
#include "knn.hip"
#include "mesh.hip"
#include "fields.hip"
#include "bookkeeping.hip"
#include "optim.hip"
#include "lbs.hip"
#include "pose.hip"
#include "step_images.hip"
#include "photometric.hip"
#include "surface.hip"
#include "meshview.hip"
#include "meshclean.hip"

// render_bwd.hip is a separate translation unit (different optimisation flags)
extern "C" __global__ void hgs_k_render_bwd(View, Layout, const hgs_status*, const SortRec*, const float*,
                                            const float*, const float*, const float*, const float*,
                                            const float*, const float*, float*, uint32_t);
extern "C" __global__ void hgs_k_pair_reduce_em(View, Layout, const hgs_status*, const SortRec*, const float*, float*, uint32_t, uint32_t);
extern "C" __global__ void hgs_k_pair_reduce_ch(View, Layout, const hgs_status*, const SortRec*, const float*, float*, uint32_t, uint32_t);

namespace {

// Experiment knobs (environment variables, rounds 3-4) exist only in -DHGS_KNOBS builds; the product library never reads the environment.
#ifdef HGS_KNOBS
inline int hgs_knob(const char* name, int dflt) { const char* e = getenv(name); return (e && atoi(e) > 0) ? atoi(e) : dflt; }
#else
inline int hgs_knob(const char*, int dflt) { return dflt; }
#endif

#define HGS_CHUNK_ROWS_MIN_VIEWS 3     // calls with at least this many views keep the backward's pair rows chunk-cell-major (entryrec.h::hgs_rec_tag)
#ifndef HGS_PRE_BWD_VPAR_MIN_VIEWS     // (a test build sets it above HGS_MAX_VIEWS: every multi-view call then takes the loop form)
#define HGS_PRE_BWD_VPAR_MIN_VIEWS 2   // calls with at least this many views run the per-Gaussian backward with one thread per
                                       // (Gaussian, view); fewer: one thread per Gaussian
#endif
constexpr size_t ALIGN = 256;
// carves one buffer into ALIGN-aligned pieces: take() -> the piece's offset; `off` ends as the buffer's size
struct Carver {
  size_t off = 0;
  size_t take(size_t bytes) { const size_t o = off; off = hgs_align_up(off + bytes, ALIGN); return o; }
};
// the device-wide scan of gridscan.h over n elements of elem bytes: its workgroups and the bytes of its block totals
struct ScanShape { unsigned blocks; size_t bsum_bytes; };
inline ScanShape scan_shape(size_t n, size_t elem) {
  const size_t nb = (n + HGS_SCAN_BLOCK - 1) / HGS_SCAN_BLOCK;
  return {(unsigned)nb, (nb + 1) * elem};
}
constexpr size_t HGS_LDS_BINS_MAX = 16384;   // T*4 bytes of LDS <= 64 KB
#define HGS_BIN_WGS_PER_VIEW_MAX 512   // (256 until round 5: at 500k Gaussians a workgroup then walked 8 chunks one after the other -
                                       //  preprocess_fwd 70 -> 54 us with 512, +2 us in `tiles` (twice the histogram rows); 100k: +-0)
#define HGS_BIN_WGS_TOTAL_MAX 1024
constexpr int HGS_MAX_BIN_WGS_PER_VIEW = HGS_BIN_WGS_PER_VIEW_MAX;
constexpr int HGS_BIN_WGS_TOTAL = HGS_BIN_WGS_TOTAL_MAX;      // binning workgroups of a batch (all views)

struct GeomCarve {
  size_t geom, tile_n, tile_start, tile_order, tile_rec, cell_info, items_part, fwd_cells,
      hist, tile_gbase, tile_count, chunk_sums, chunk_base, ctr, status, total;
};

inline int grid_dim(int pixels) { return (pixels + HGS_TILE - 1) / HGS_TILE; }

// binning workgroups per view / chunks per workgroup for a batch of B views of P Gaussians
inline void bin_shape(int B, int P, int& nblk, int& cpw, int& nwg) {
  nblk = (P + HGS_BLOCK - 1) / HGS_BLOCK;
  int want = HGS_BIN_WGS_TOTAL / (B > 0 ? B : 1);
  if (want > HGS_MAX_BIN_WGS_PER_VIEW) want = HGS_MAX_BIN_WGS_PER_VIEW;
  if (want < 1) want = 1;
  cpw = (nblk + want - 1) / want;
  if (cpw < 1) cpw = 1;
  nwg = (nblk + cpw - 1) / cpw;
}

GeomCarve carve_geom(int B, int P, int H, int W) {
  const size_t T = (size_t)grid_dim(W) * grid_dim(H);
  const size_t TT = T * (size_t)B;
  int nblk, cpw, nwg;
  bin_shape(B, P, nblk, cpw, nwg);
  const bool lds = T <= HGS_LDS_BINS_MAX;
  GeomCarve c;
  Carver cv;
  c.geom = cv.take((size_t)B * P * sizeof(GeomRec));
  c.tile_n = cv.take(TT * 4);
  c.tile_start = cv.take(TT * 4);
  c.tile_order = cv.take(TT * 4);
  c.tile_rec = cv.take(TT * 16);
  c.cell_info = cv.take(TT * 16 * sizeof(CellInfo));
  const size_t dcap = hgs_die_cells((int)TT);            // work tables are per die (Counters::sched)
  c.items_part = cv.take(HGS_NXCD * 2 * dcap * sizeof(uint4));   // last (partial) segment of every cell list, by length class
  c.fwd_cells = cv.take((size_t)HGS_NXCD * HGS_NFC * dcap * 4);    // non-empty cells by length class
  c.hist = cv.take(lds ? (size_t)B * nwg * T * 4 : 0);
  c.tile_gbase = cv.take(lds ? (size_t)HGS_ROW_GROUPS * TT * 4 : 0);
  c.tile_count = cv.take(lds ? 0 : TT * 4);
  c.chunk_sums = cv.take((size_t)B * nblk * 4);
  c.chunk_base = cv.take((size_t)B * nblk * 4);
  c.ctr = cv.take(sizeof(Counters));
  c.status = cv.take(sizeof(hgs_status));
  c.total = cv.off;
  return c;
}

struct BinCarve { size_t keys, recs, cell_list, entpair, cstate, items_full, total; };

// Pair-sized arrays hold HGS_PAIRS_PER_ENTRY slots per entry of capacity: an entry can reach all 16 cells of
// its tile (zoomed-in cameras), so no second capacity (and no second overflow path) exists.
BinCarve carve_bin(int64_t cap) {
  BinCarve c;
  Carver cv;
  const size_t C = (size_t)(cap > 0 ? cap : 0);
  const size_t NP = C * HGS_PAIRS_PER_ENTRY;
  c.keys = cv.take(C * 8);
  c.recs = cv.take(C * sizeof(SortRec));
  c.cell_list = cv.take(NP * 8);
  c.entpair = cv.take(C * 8);
  // a cell list of len entries has ceil(len / HGS_SEGLEN) - 1 stored states and ceil(len / HGS_SEGLEN) work items, len / HGS_SEGLEN of them full
  c.cstate = cv.take((NP / HGS_SEGLEN + 1) * HGS_CSTATE_FLOATS * sizeof(float));
  c.items_full = cv.take(HGS_NXCD * (NP / HGS_SEGLEN + 1) * sizeof(uint4));     // per die; one die's tiles may hold (nearly) all full segments
  c.total = cv.off;
  return c;
}

Layout make_layout(void* geom, void* bin, void* img, int B, int P, int H, int W, int64_t cap) {
  const GeomCarve g = carve_geom(B, P, H, W);
  const BinCarve b = carve_bin(cap);
  char* gp = static_cast<char*>(geom);
  char* bp = static_cast<char*>(bin);
  Layout L;
  L.geom = reinterpret_cast<GeomRec*>(gp + g.geom);
  L.tile_n = reinterpret_cast<uint32_t*>(gp + g.tile_n);
  L.tile_start = reinterpret_cast<uint32_t*>(gp + g.tile_start);
  L.tile_order = reinterpret_cast<uint32_t*>(gp + g.tile_order);
  L.tile_rec = reinterpret_cast<uint4*>(gp + g.tile_rec);
  L.cell_info = reinterpret_cast<CellInfo*>(gp + g.cell_info);
  L.items_part = reinterpret_cast<uint4*>(gp + g.items_part);
  L.fwd_cells = reinterpret_cast<uint32_t*>(gp + g.fwd_cells);
  L.hist = reinterpret_cast<uint32_t*>(gp + g.hist);
  L.tile_gbase = reinterpret_cast<uint32_t*>(gp + g.tile_gbase);
  L.tile_count = reinterpret_cast<uint32_t*>(gp + g.tile_count);
  L.chunk_sums = reinterpret_cast<uint32_t*>(gp + g.chunk_sums);
  L.chunk_base = reinterpret_cast<uint32_t*>(gp + g.chunk_base);
  L.ctr = reinterpret_cast<Counters*>(gp + g.ctr);
  L.keys = bp ? reinterpret_cast<unsigned long long*>(bp + b.keys) : nullptr;
  L.recs = bp ? reinterpret_cast<SortRec*>(bp + b.recs) : nullptr;
  L.cell_list = bp ? reinterpret_cast<uint2*>(bp + b.cell_list) : nullptr;
  L.entpair = bp ? reinterpret_cast<uint2*>(bp + b.entpair) : nullptr;
  L.cstate = bp ? reinterpret_cast<float*>(bp + b.cstate) : nullptr;
  L.items_full = bp ? reinterpret_cast<uint4*>(bp + b.items_full) : nullptr;
  L.full_cap = (uint32_t)((size_t)(cap > 0 ? cap : 0) * HGS_PAIRS_PER_ENTRY / HGS_SEGLEN + 1);
  L.n_contrib = static_cast<uint32_t*>(img);
  return L;
}

View make_view(const hgs_settings* s, int B, int P, int M, int64_t cap, int max_tile_hint = 0, int act = 0) {
  View v;
  v.act = act;
  v.pairchunks = B >= HGS_CHUNK_ROWS_MIN_VIEWS ? 1 : 0;
  for (int b = 0; b < HGS_MAX_VIEWS; ++b) {
    const hgs_settings& sb = s[b < B ? b : 0];
    Cam& c = v.cam[b];
    c.viewmatrix = sb.viewmatrix;
    c.projmatrix = sb.projmatrix;
    c.campos = sb.campos;
    c.bg = sb.bg;
    c.tanfovx = sb.tanfovx;
    c.tanfovy = sb.tanfovy;
    c.focal_x = (float)sb.image_width / (2.0f * sb.tanfovx);
    c.focal_y = (float)sb.image_height / (2.0f * sb.tanfovy);
  }
  v.scale_modifier = s->scale_modifier;
  v.W = s->image_width;
  v.H = s->image_height;
  v.grid_x = grid_dim(v.W);
  v.grid_y = grid_dim(v.H);
  v.T = v.grid_x * v.grid_y;
  v.B = B;
  v.TT = B * v.T;
  v.P = P;
  v.M = M;
  v.D = s->sh_degree;
  v.lds_bins = (size_t)v.T <= HGS_LDS_BINS_MAX ? 1 : 0;
  bin_shape(B, P, v.nblk, v.cpw, v.nwg);
  if (!v.lds_bins) { v.cpw = 1; v.nwg = v.nblk; }
  v.entry_capacity = (uint32_t)(cap < 0 ? 0 : (cap > 0xffffffffll ? 0xffffffffll : cap));
  v.max_tile_hint = max_tile_hint;
  return v;
}

inline int hip_rc(hipError_t e) { return e == hipSuccess ? HGS_OK : -(1000 + (int)e); }

// A header that holds a box as ordered-key images (gridscan.h): all of it zero, the box empty (bmin = all ones, bmax = 0).
// (KnnGrid's other fields are zeroed with it; hgs_k_knn_grid_setup writes every one of them before anything reads it.)
inline hipError_t box_init(void* hdr, size_t hdr_bytes, uint32_t* bmin, hipStream_t stream) {
  const hipError_t e = hipMemsetAsync(hdr, 0, hdr_bytes, stream);
  return e != hipSuccess ? e : hipMemsetAsync(bmin, 0xff, 3 * sizeof(uint32_t), stream);
}

#define HGS_LAUNCH_CHECK()                       \
  do {                                           \
    hipError_t e__ = hipGetLastError();          \
    if (e__ != hipSuccess) return hip_rc(e__);   \
  } while (0)

#define HGS_STAGE(k)                                                              \
  do {                                                                            \
    if (stage_events && stage_events[k]) {                                        \
      hipError_t e__ = hipEventRecord(static_cast<hipEvent_t>(stage_events[k]), stream); \
      if (e__ != hipSuccess) return hip_rc(e__);                                  \
    }                                                                             \
  } while (0)

// The long-list sort classes (one 1024-thread workgroup per tile of more than 4 096 entries: hgs_k_sort_large / _huge) run
// BESIDE the LDS class on a per-device side stream - fork behind `fill`, join in front of the blend.  A view of 500k
// Gaussians has one or two such tiles; launched in front of hgs_k_sort_lds on the caller's stream they held the whole
// GPU for the 39 us one of them takes (8 % of that step).  The classes write disjoint tiles and share only the bump
// allocators (atomics), so they may overlap.  The side stream and its two events are created once per device; a device
// where that fails keeps the launches on the caller's stream.  Calls whose hint rules the classes out never touch it.
struct SideStream {
  std::mutex mu;
  hipStream_t s = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
  bool tried = false, ok = false;
};

// Everything the host remembers per device, looked up once per call by the STREAM's device (not the thread's current
// one).  One failure rule: a stream whose device cannot be determined has no state (device_state() == nullptr), and every
// reader below then gives its most conservative answer - 256 CUs, no side stream, no LDS raise (=> the loop form of the
// per-Gaussian backward); no other device's entry is read or written.
struct DeviceState {
  std::atomic<int> cus;                             // 0: not asked yet
  SideStream side;
  std::atomic<int> lds_raised[HGS_PRE_BWD_ROWS];    // per row of hgs_pre_bwd_forms: 0 not tried, 1 raised to 160 KB, -1 refused
};
DeviceState g_devices[64];
DeviceState* device_state(hipStream_t stream) {
  int dev = 0;
  if (hipStreamGetDevice(stream, &dev) != hipSuccess || dev < 0 || dev >= 64) { (void)hipGetLastError(); return nullptr; }
  return &g_devices[dev];
}
// the state's device made current (stream / event creation and function attributes act on the current device); the
// caller's comes back at the end of the scope.  !ok (the current device cannot be read or switched): the same failure
// rule - the caller creates / raises nothing rather than act on a device it does not know
struct DeviceCurrent {
  int dev, cur = 0;
  bool ok, switched;
  explicit DeviceCurrent(const DeviceState* ds)
      : dev((int)(ds - g_devices)), ok(hipGetDevice(&cur) == hipSuccess), switched(ok && cur != dev) {
    if (switched) ok = hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceCurrent() { if (switched) (void)hipSetDevice(cur); }
};

// CUs of the stream's device (persistent grids are sized by it)
int cu_count(DeviceState* ds) {
  if (!ds) return 256;
  int cus = ds->cus.load(std::memory_order_relaxed);
  if (cus > 0) return cus;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, (int)(ds - g_devices)) != hipSuccess || cus < 1) cus = 256;
  ds->cus.store(cus, std::memory_order_relaxed);
  return cus;
}

// the device's side stream and its two events, created at the first call that wants them; nullptr: stay on the caller's stream
SideStream* side_stream(DeviceState* ds) {
  if (!ds) return nullptr;
  SideStream& t = ds->side;
  std::lock_guard<std::mutex> lk(t.mu);
  if (!t.tried) {
    t.tried = true;
    DeviceCurrent on(ds);
    t.ok = on.ok && hipStreamCreateWithFlags(&t.s, hipStreamNonBlocking) == hipSuccess &&
           hipEventCreateWithFlags(&t.fork, hipEventDisableTiming) == hipSuccess &&
           hipEventCreateWithFlags(&t.join, hipEventDisableTiming) == hipSuccess;
    if (!t.ok) (void)hipGetLastError();
  }
  return t.ok ? &t : nullptr;
}

// May row `row` of hgs_pre_bwd_forms be launched with more than 64 KB of dynamic LDS on this device?  The attribute
// is raised ONCE per (device, row) to the CU's whole LDS and remembered: a driver call per backward was host time on the
// hot path; a refusal is remembered too (and said once on stderr): the loop form then serves.
bool pre_bwd_lds_raised(DeviceState* ds, int row) {
  if (!ds) return false;
  int st = ds->lds_raised[row].load(std::memory_order_relaxed);
  if (st == 0) {
    const PreBwdForm& form = hgs_pre_bwd_forms.row[row];
    DeviceCurrent on(ds);
    if (on.ok && hipFuncSetAttribute(reinterpret_cast<const void*>(form.kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess) {
      st = 1;
    } else {
      (void)hipGetLastError();
      st = -1;
      fprintf(stderr, "libhgs_rast: cannot raise the dynamic LDS limit of %s on device %d: "
                      "batches that need more than 64 KB take the (slower) loop form\n", form.name, on.dev);
    }
    ds->lds_raised[row].store(st, std::memory_order_relaxed);
  }
  return st > 0;
}

bool settings_ok(const hgs_settings* s) {
  return s && s->image_height > 0 && s->image_width > 0 && s->bg && s->viewmatrix &&
         s->projmatrix && s->campos && s->sh_degree >= 0 && s->sh_degree <= 3 &&
         s->image_width <= 16 * 65535 && s->image_height <= 16 * 65535;
}

// a batch: 1..HGS_MAX_VIEWS valid settings that agree in everything that is not per camera
bool batch_ok(const hgs_settings* s, int B) {
  if (!s || B < 1 || B > HGS_MAX_VIEWS) return false;
  for (int b = 0; b < B; ++b) {
    if (!settings_ok(s + b)) return false;
    if (s[b].image_height != s[0].image_height || s[b].image_width != s[0].image_width ||
        s[b].sh_degree != s[0].sh_degree || s[b].scale_modifier != s[0].scale_modifier)
      return false;
  }
  return (size_t)B * grid_dim(s->image_width) * grid_dim(s->image_height) < (1u << 30);
}

}  // namespace

#ifdef HGS_TIMELINE
// debug builds only: copy one kernel's timeline table to the host (synchronous) and clear it
extern "C" int hgs_debug_timeline_read(int kernel_id, void* host_dst) {
  if (kernel_id < 0 || kernel_id >= HGS_TL_KERNELS) return -1;
  const size_t bytes = sizeof(unsigned long long) * HGS_TL_SLOTS * 4, off = bytes * (size_t)kernel_id;
  if (hipDeviceSynchronize() != hipSuccess) return -2;
  if (hipMemcpyFromSymbol(host_dst, HIP_SYMBOL(hgs_tl), bytes, off, hipMemcpyDeviceToHost) != hipSuccess) return -3;
  void* p = nullptr;
  if (hipGetSymbolAddress(&p, HIP_SYMBOL(hgs_tl)) != hipSuccess) return -4;
  return hipMemset(static_cast<char*>(p) + off, 0, bytes) == hipSuccess ? 0 : -5;
}
#endif

extern "C" {

int hgs_knn_mean_dist2(int32_t P, const float* points, float* mean_dist2, void* stream_) {
  if (P < 0) return HGS_EINVAL;
  if (P == 0) return HGS_OK;
  if (!points || !mean_dist2) return HGS_EINVAL;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(hgs_k_knn3, dim3((P + 255) / 256), dim3(256), 0, stream, (int)P, points, mean_dist2,
                     static_cast<const KnnGrid*>(nullptr));
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

namespace {
struct KnnCarve { size_t grid, cell_of, count, cursor, bsum, sorted, total; uint32_t nc_max; };
KnnCarve carve_knn(int32_t P) {
  KnnCarve c;
  const size_t n = (size_t)(P > 0 ? P : 0);
  const size_t want = std::max<size_t>(64, 2 * n);
  c.nc_max = (uint32_t)std::min<size_t>(want, HGS_KNN_MAX_CELLS);
  Carver cv;
  c.grid = cv.take(sizeof(KnnGrid));
  c.cell_of = cv.take(n * 4);
  c.count = cv.take(((size_t)c.nc_max + 1) * 4);
  c.cursor = cv.take((size_t)c.nc_max * 4);
  c.bsum = cv.take(scan_shape((size_t)c.nc_max + 1, 4).bsum_bytes);        // (sized like count[]: with the end sentinel)
  c.sorted = cv.take(n * 16);
  c.total = cv.off;
  return c;
}
}  // namespace

size_t hgs_knn_scratch_bytes(int32_t P) { return carve_knn(P).total; }

int hgs_knn_mean_dist2_grid(int32_t P, const float* points, float* mean_dist2, void* scratch, void* stream_) {
  if (P < 0) return HGS_EINVAL;
  if (P == 0) return HGS_OK;
  if (!points || !mean_dist2 || !scratch) return HGS_EINVAL;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const KnnCarve c = carve_knn(P);
  char* sp = static_cast<char*>(scratch);
  KnnGrid* G = reinterpret_cast<KnnGrid*>(sp + c.grid);
  uint32_t* cell_of = reinterpret_cast<uint32_t*>(sp + c.cell_of);
  uint32_t* count = reinterpret_cast<uint32_t*>(sp + c.count);
  uint32_t* cursor = reinterpret_cast<uint32_t*>(sp + c.cursor);
  uint32_t* bsum = reinterpret_cast<uint32_t*>(sp + c.bsum);
  float4* sorted = reinterpret_cast<float4*>(sp + c.sorted);
  hipError_t e = box_init(G, sizeof(KnnGrid), G->bmin, stream);
  if (e == hipSuccess) e = hipMemsetAsync(count, 0, ((size_t)c.nc_max + 1) * 4, stream);      // cell counters
  if (e != hipSuccess) return hip_rc(e);
  const unsigned gp = (unsigned)((P + 255) / 256), gc = scan_shape(c.nc_max, 4).blocks;
  hipLaunchKernelGGL(hgs_k_knn_bbox, dim3(gp), dim3(256), 0, stream, (int)P, points, G);
  hipLaunchKernelGGL(hgs_k_knn_grid_setup, dim3(1), dim3(64), 0, stream, (int)P, c.nc_max, G);
  hipLaunchKernelGGL(hgs_k_knn_count, dim3(gp), dim3(256), 0, stream, (int)P, points, (const KnnGrid*)G, cell_of, count);
  hipLaunchKernelGGL(hgs_k_knn_scan1, dim3(gc), dim3(1024), 0, stream, (const KnnGrid*)G, (const uint32_t*)count, bsum);
  hipLaunchKernelGGL(hgs_k_knn_scan2, dim3(1), dim3(1024), 0, stream, (const KnnGrid*)G, bsum);
  hipLaunchKernelGGL(hgs_k_knn_scan3, dim3(gc), dim3(1024), 0, stream, (int)P, G, count, cursor, (const uint32_t*)bsum);
  hipLaunchKernelGGL(hgs_k_knn_scatter, dim3(gp), dim3(256), 0, stream, (int)P, points, (const uint32_t*)cell_of, cursor, sorted);
  hipLaunchKernelGGL(hgs_k_knn_search, dim3(gp), dim3(256), 0, stream, (int)P, (const KnnGrid*)G, (const uint32_t*)count,
                     (const float4*)sorted, mean_dist2);
  // degenerate clouds (decided on the device: KnnGrid::brute): the exact brute force; returns at once otherwise
  hipLaunchKernelGGL(hgs_k_knn3, dim3(gp), dim3(256), 0, stream, (int)P, points, mean_dist2, (const KnnGrid*)G);
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

int hgs_reduce_view_packs_acc(int32_t world, int64_t P, int32_t F, const float* gathered, const float* acc_in,
                              float* out, void* stream_) {
  if (world < 1 || P < 0 || F < 1) return HGS_EINVAL;
  if (P == 0) return HGS_OK;
  if (!gathered || !out) return HGS_EINVAL;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const long long n = (long long)P * F;
  hipLaunchKernelGGL(hgs_k_reduce_view_packs, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                     (int)world, n, (int)F, gathered, acc_in, out);
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

int hgs_reduce_view_packs_unpack(int32_t world, int64_t P, int32_t M, const float* gathered, const float* acc_in,
                                 float* g_means3D, float* g_means2D, float* g_sh, float* g_opac, float* g_scales,
                                 float* g_rot, int32_t* radii, void* stream_) {
  if (world < 1 || P < 0 || M < 0) return HGS_EINVAL;
  if (P == 0) return HGS_OK;
  if (!gathered || !g_means3D || !g_means2D || (M > 0 && !g_sh) || !g_opac || !g_scales || !g_rot || !radii) return HGS_EINVAL;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int F = 15 + 3 * M;
  const long long n = (long long)P * F;
  hipLaunchKernelGGL(hgs_k_reduce_view_packs_unpack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                     (int)world, n, (int)F, (int)M, gathered, acc_in, g_means3D, g_means2D, g_sh, g_opac, g_scales, g_rot, radii);
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

int hgs_reduce_view_packs(int32_t world, int64_t P, int32_t F, const float* gathered, float* out,
                          void* stream_) {
  return hgs_reduce_view_packs_acc(world, P, F, gathered, nullptr, out, stream_);
}

int hgs_pack_view_contribution(int32_t P, int32_t M, const float* g_means3D, const float* g_means2D,
                               const float* g_sh, const float* g_opac, const float* g_scales,
                               const float* g_rot, const int32_t* radii, float* out, void* stream_) {
  if (P < 0 || M < 0) return HGS_EINVAL;
  if (P == 0) return HGS_OK;
  if (!g_means3D || !g_means2D || (M > 0 && !g_sh) || !g_opac || !g_scales || !g_rot || !radii || !out)
    return HGS_EINVAL;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const long long n = (long long)P * (15 + 3 * M);
  hipLaunchKernelGGL(hgs_k_pack_view_contribution, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                     (int)P, (int)M, g_means3D, g_means2D, g_sh, g_opac, g_scales, g_rot, radii, out);
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

int hgs_abi_version(void) { return 17; }

size_t hgs_geom_bytes_batch(int32_t B, int32_t P, int32_t H, int32_t W) {
  if (B < 1 || B > HGS_MAX_VIEWS || P < 0 || H <= 0 || W <= 0) return 0;
  return carve_geom(B, P, H, W).total;
}
size_t hgs_geom_bytes(int32_t P, int32_t H, int32_t W) { return hgs_geom_bytes_batch(1, P, H, W); }
size_t hgs_bin_bytes(int64_t entry_capacity) { return carve_bin(entry_capacity).total; }
size_t hgs_img_bytes_batch(int32_t B, int32_t H, int32_t W) {
  if (B < 1 || B > HGS_MAX_VIEWS || H <= 0 || W <= 0) return 0;
  return hgs_align_up((size_t)B * H * W * 4, ALIGN);
}
size_t hgs_img_bytes(int32_t H, int32_t W) { return hgs_img_bytes_batch(1, H, W); }
// one gradient row per entry + one per (entry, cell) pair
size_t hgs_bwd_scratch_bytes(int64_t R) {
  return hgs_align_up((size_t)(R > 0 ? R : 0) * (HGS_ROW_FLOATS + HGS_PAIRS_PER_ENTRY * HGS_PROW_FLOATS) * sizeof(float), ALIGN);
}
size_t hgs_bwd_scratch_bytes_pairs(int64_t R, int64_t pairs) {
  if (R <= 0) return 0;
  if (pairs <= 0 || pairs > R * HGS_PAIRS_PER_ENTRY) return hgs_bwd_scratch_bytes(R);
  return hgs_align_up(((size_t)R * HGS_ROW_FLOATS + (size_t)pairs * HGS_PROW_FLOATS) * sizeof(float), ALIGN);
}

int hgs_forward_batch_act(const hgs_settings* s, int32_t B, int32_t P, int32_t M, const float* means3D,
                          const float* shs, const float* colors_precomp, const float* opacities,
                          const float* scales, const float* rotations, const float* cov3D_precomp,
                          float* out_color, float* out_depth, float* out_alpha, int32_t* radii,
                          void* geom, void* bin, int64_t entry_capacity, void* img,
                          int32_t store_bwd_state, int32_t max_tile_entries_hint, hgs_status* status_host,
                          int32_t status_host_mapped, void* status_event, void* const* stage_events,
                          int32_t activation_flags, void* stream_) {
  return hgs_forward_batch_act_leaf(s, B, P, M, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                    out_color, out_depth, out_alpha, radii, geom, bin, entry_capacity, img, store_bwd_state,
                                    max_tile_entries_hint, status_host, status_host_mapped, status_event, stage_events,
                                    activation_flags, nullptr, stream_);
}

int hgs_forward_batch_act_leaf(const hgs_settings* s, int32_t B, int32_t P, int32_t M, const float* means3D,
                               const float* shs, const float* colors_precomp, const float* opacities,
                               const float* scales, const float* rotations, const float* cov3D_precomp,
                               float* out_color, float* out_depth, float* out_alpha, int32_t* radii,
                               void* geom, void* bin, int64_t entry_capacity, void* img,
                               int32_t store_bwd_state, int32_t max_tile_entries_hint, hgs_status* status_host,
                               int32_t status_host_mapped, void* status_event, void* const* stage_events,
                               int32_t activation_flags, float* means2D_leaf, void* stream_) {
  if (activation_flags & ~(7 | HGS_GRAD_SCALE_TRUE_DERIVATIVE | HGS_ANTIALIAS)) return HGS_EINVAL;      // (the gradient bit is the backward's: ignored here)
  if (!batch_ok(s, B) || P < 0 || !out_color || !out_depth || !out_alpha || !geom || !img ||
      entry_capacity < 0)
    return HGS_EINVAL;
  if (P > 0) {
    if (!means3D || !opacities || !radii) return HGS_EINVAL;
    if ((shs != nullptr) == (colors_precomp != nullptr)) return HGS_ESHAPE;
    const bool has_sr = scales != nullptr && rotations != nullptr;
    if ((scales != nullptr) != (rotations != nullptr)) return HGS_ESHAPE;
    if (has_sr == (cov3D_precomp != nullptr)) return HGS_ESHAPE;
    if (shs && M < (s->sh_degree + 1) * (s->sh_degree + 1)) return HGS_ESHAPE;
    if (entry_capacity > 0 && !bin) return HGS_EINVAL;
    if ((int64_t)B * P >= (1ll << 31) || P >= (1 << 28)) return HGS_EINVAL;
  }
  // entry ids travel in HGS_ENTRY_BITS bits (entpair.x, entryrec.h::hgs_entpair_x): a larger list cannot be addressed
  if (entry_capacity > HGS_MAX_ENTRY_CAPACITY) return HGS_EINVAL;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  DeviceState* const ds = device_state(stream);
  const int ncu = cu_count(ds);
  // (the gradient bit belongs to the backward: masked out, so that no forward kernel can ever branch on it; the
  // antialiasing bit selects the forward kernel, not a branch in it)
  const bool aa = (activation_flags & HGS_ANTIALIAS) != 0;
  const View v = make_view(s, B, P, M, entry_capacity, max_tile_entries_hint > 0 ? max_tile_entries_hint : 0,
                           activation_flags & 7);
  const Layout L = make_layout(geom, bin, img, B, P, v.H, v.W, entry_capacity);
  hgs_status* status_dev =
      reinterpret_cast<hgs_status*>(static_cast<char*>(geom) + carve_geom(B, P, v.H, v.W).status);

  HGS_STAGE(0);
  hipError_t e = hipSuccess;
  if (v.nblk == 0) {       // no preprocess launch (P == 0): nobody else zeroes the counters
    e = hipMemsetAsync(L.ctr, 0, sizeof(Counters), stream);
    if (e != hipSuccess) return hip_rc(e);
  }
  const size_t lds_bytes = (size_t)v.T * 4;
  if (!v.lds_bins) {
    e = hipMemsetAsync(L.tile_count, 0, (size_t)v.TT * 4, stream);
    if (e != hipSuccess) return hip_rc(e);
  }
  if (v.nblk > 0) {
    if (v.lds_bins)
      hipLaunchKernelGGL(aa ? hgs_k_preprocess_fwd_aa : hgs_k_preprocess_fwd, dim3(v.B * v.nwg), dim3(HGS_BLOCK), lds_bytes,
                         stream, v, L, means3D, shs, colors_precomp, opacities, scales, rotations,
                         cov3D_precomp, radii, means2D_leaf);
    else
      hipLaunchKernelGGL(aa ? hgs_k_preprocess_fwd_ga_aa : hgs_k_preprocess_fwd_ga, dim3(v.B * v.nblk), dim3(HGS_BLOCK), 0,
                         stream, v, L, means3D, shs, colors_precomp, opacities, scales, rotations,
                         cov3D_precomp, radii, means2D_leaf);
    HGS_LAUNCH_CHECK();
  }
  HGS_STAGE(1);
  // tile tables: 64 tiles per workgroup, all views in one launch
  const unsigned bpv = (unsigned)((v.T + HGS_TILES_PER_WG - 1) / HGS_TILES_PER_WG);
  hipLaunchKernelGGL(hgs_k_tiles, dim3(bpv * (unsigned)v.B), dim3(64 * HGS_ROW_GROUPS), 0, stream, v, L);
  HGS_LAUNCH_CHECK();
  HGS_STAGE(2);
  // binning workgroups scatter the keys; `order_wgs` more place the tiles into tile_order, hand out
  // the chunks' entry-id bases and publish the status (device copy, pinned host mirror)
  const unsigned order_wgs = (unsigned)((v.TT + HGS_BLOCK - 1) / HGS_BLOCK);
  hgs_status* status_mapped = status_host_mapped ? status_host : nullptr;
  const unsigned nbin = entry_capacity > 0 ? (unsigned)(v.B * (v.lds_bins ? v.nwg : v.nblk)) : 0u;
  if (v.lds_bins && nbin)
    hipLaunchKernelGGL(hgs_k_fill, dim3(nbin + order_wgs), dim3(HGS_BLOCK), lds_bytes, stream, v, L, status_dev,
                       status_mapped, (int)nbin);
  else
    hipLaunchKernelGGL(hgs_k_fill_ga, dim3(nbin + order_wgs), dim3(HGS_BLOCK), 0, stream, v, L, status_dev,
                       status_mapped, (int)nbin);
  HGS_LAUNCH_CHECK();
  // the status is final here: publish it now so the host can wait for it alone
  if (status_host && !status_host_mapped) {
    e = hipMemcpyAsync(status_host, status_dev, sizeof(hgs_status), hipMemcpyDeviceToHost, stream);
    if (e != hipSuccess) return hip_rc(e);
  }
  if (status_event) {
    e = hipEventRecord(static_cast<hipEvent_t>(status_event), stream);
    if (e != hipSuccess) return hip_rc(e);
  }
  if (entry_capacity > 0) {
    HGS_STAGE(3);
    // tiles are ordered heavy-first, so a class with more than LO entries per tile can only
    // occupy the first capacity/LO positions of tile_order
    auto class_grid = [&](int64_t lo) {
      const int64_t g = entry_capacity / lo + 1;
      return (unsigned)(g < v.TT ? g : v.TT);
    };
    // the caller's hint (longest tile list it has seen, with margin) lets us skip launching
    // sort classes that cannot occur; a wrong hint is caught on the device (overflow bit 2).
    const int hint = v.max_tile_hint;
    const bool need_huge = hint <= 0 || hint > 16384, need_large = hint <= 0 || hint > HGS_SORT_LDS_MAX;
    // (the side stream costs a cross-stream edge, ~11 us at the join: it is taken when a long list is EXPECTED - a hint
    // beyond 1.5 x the class boundary, i.e. a list the caller has seen, not the margin on a shorter one - or unknown)
    const bool expect_long = hint <= 0 || hint > HGS_SORT_LDS_MAX + HGS_SORT_LDS_MAX / 2 + 64;
    SideStream* side = ((need_huge || need_large) && expect_long) ? side_stream(ds) : nullptr;
    {
      std::unique_lock<std::mutex> side_lk;
      hipStream_t s2 = stream;
      if (side) {                                        // fork: the long-list classes wait for `fill`, nothing else
        side_lk = std::unique_lock<std::mutex>(side->mu);
        e = hipEventRecord(side->fork, stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(side->s, side->fork, 0);
        if (e != hipSuccess) return hip_rc(e);
        s2 = side->s;
      }
      if (need_huge) {
        hipLaunchKernelGGL(hgs_k_sort_huge, dim3(class_grid(16384)), dim3(1024), 0, s2, v, L, status_dev);
        HGS_LAUNCH_CHECK();
      }
      if (need_large) {
        hipLaunchKernelGGL(hgs_k_sort_large, dim3(class_grid(HGS_SORT_LDS_MAX)), dim3(1024), 0, s2, v, L, status_dev);
        HGS_LAUNCH_CHECK();
      }
      if (side) {
        e = hipEventRecord(side->join, side->s);
        if (e != hipSuccess) return hip_rc(e);
      }
      // persistent workgroups (53 KB of LDS: three per CU), tiles heavy first round-robin
      const unsigned sort_wgs = std::min<unsigned>(class_grid(1), (unsigned)(hgs_knob("HGS_SORT_WGS_PER_CU", 3) * ncu));
      hipLaunchKernelGGL(v.pairchunks ? hgs_k_sort_lds_ch : hgs_k_sort_lds, dim3(sort_wgs), dim3(HGS_SORT_NT), 0, stream, v, L,
                         status_dev);
      HGS_LAUNCH_CHECK();
      if (side) {                                        // join: the blend needs every class
        e = hipStreamWaitEvent(stream, side->join, 0);
        if (e != hipSuccess) return hip_rc(e);
      }
    }
  } else {
    HGS_STAGE(3);
  }
  HGS_STAGE(4);
  // Blend: waves of four cells of one length class, longest first, then the background of the empty cells
  // (render_fwd.hip).  Non-empty cells <= min(16 B T, pairs): a capacity bound, surplus waves leave at once.
  {
    // persistent cell waves: enough to fill the chip (4 waves per block; 4 blocks per CU), never more than the cells
    const int64_t cells = std::min<int64_t>((int64_t)16 * v.TT, (int64_t)HGS_PAIRS_PER_ENTRY * entry_capacity);
    // (the snake schedule of hgs_k_render_fwd visits every item only when the block count is a multiple of 4)
    const int64_t fwd_blocks = (int64_t)hgs_knob("HGS_FWD_BLOCKS_PER_CU", 4) * ncu;
    const unsigned cell_blocks = (unsigned)std::max<int64_t>(4, std::min<int64_t>(fwd_blocks, (cells + 3) / 4) & ~int64_t(3));
    const unsigned bg_blocks = (unsigned)v.TT;
    hipLaunchKernelGGL(store_bwd_state ? hgs_k_render_fwd_store : hgs_k_render_fwd_nostore, dim3(cell_blocks + bg_blocks),
                       dim3(HGS_FWD_THREADS), 0, stream, v, L, cell_blocks, status_dev, status_mapped, L.recs, L.cstate,
                       out_color, out_depth, out_alpha);
  }
  HGS_LAUNCH_CHECK();
  HGS_STAGE(5);
  return HGS_OK;
}

int hgs_forward_batch(const hgs_settings* s, int32_t B, int32_t P, int32_t M, const float* means3D,
                      const float* shs, const float* colors_precomp, const float* opacities,
                      const float* scales, const float* rotations, const float* cov3D_precomp,
                      float* out_color, float* out_depth, float* out_alpha, int32_t* radii,
                      void* geom, void* bin, int64_t entry_capacity, void* img,
                      int32_t store_bwd_state, int32_t max_tile_entries_hint, hgs_status* status_host,
                      int32_t status_host_mapped, void* status_event, void* const* stage_events,
                      void* stream_) {
  return hgs_forward_batch_act(s, B, P, M, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                               out_color, out_depth, out_alpha, radii, geom, bin, entry_capacity, img, store_bwd_state,
                               max_tile_entries_hint, status_host, status_host_mapped, status_event, stage_events, 0,
                               stream_);
}

int hgs_forward(const hgs_settings* s, int32_t P, int32_t M, const float* means3D,
                const float* shs, const float* colors_precomp, const float* opacities,
                const float* scales, const float* rotations, const float* cov3D_precomp,
                float* out_color, float* out_depth, float* out_alpha, int32_t* radii,
                void* geom, void* bin, int64_t entry_capacity, void* img,
                int32_t store_bwd_state, int32_t max_tile_entries_hint, hgs_status* status_host,
                int32_t status_host_mapped, void* status_event, void* const* stage_events,
                void* stream_) {
  return hgs_forward_batch(s, 1, P, M, means3D, shs, colors_precomp, opacities, scales, rotations,
                           cov3D_precomp, out_color, out_depth, out_alpha, radii, geom, bin, entry_capacity,
                           img, store_bwd_state, max_tile_entries_hint, status_host, status_host_mapped,
                           status_event, stage_events, stream_);
}

}  // extern "C"

namespace {
// the backward of a batch; `pack` != nullptr: hgs_backward_batch_packed (one (P, pack_F) row-major pack instead of the six
// parameter-gradient tensors; dL_dshs / dL_dscales / dL_drotations are then non-null MARKERS for the parts the row carries)
int backward_impl(const hgs_settings* s, int32_t B, int32_t P, int32_t M, const float* means3D,
                           const float* shs, const float* colors_precomp, const float* opacities,
                           const float* scales, const float* rotations, const float* cov3D_precomp,
                           const int32_t* radii, const float* out_color, const float* out_depth,
                           const float* out_alpha, const float* dL_dout_color,
                           const float* dL_dout_depth, const float* dL_dout_alpha, const void* geom,
                           const void* bin, const void* img, const hgs_status* status,
                           int64_t entry_capacity, void* bwd_scratch, float* dL_dmeans3D, float* dL_dmeans2D, float* dL_dshs,
                           float* dL_dcolors_precomp, float* dL_dopacities, float* dL_dscales,
                           float* dL_drotations, float* dL_dcov3D_precomp, void* const* stage_events,
                           int32_t activation_flags, float* pack, int32_t pack_F, void* stream_) {
  (void)radii;
  if (activation_flags & ~(7 | HGS_GRAD_SCALE_TRUE_DERIVATIVE | HGS_ANTIALIAS)) return HGS_EINVAL;
  if ((activation_flags & (HGS_ACT_OPACITY_SIGMOID | HGS_ANTIALIAS)) && P > 0 && !opacities) return HGS_EINVAL;
  if (!batch_ok(s, B) || P < 0 || !geom || !img || entry_capacity < 0 || entry_capacity > HGS_MAX_ENTRY_CAPACITY) return HGS_EINVAL;
  if (status && status->overflow) return HGS_EINVAL;
  if (status && (int64_t)status->reserved[0] != entry_capacity) return HGS_EINVAL;
  if (P == 0) return HGS_OK;
  if (!means3D || !out_color || !out_depth || !out_alpha) return HGS_EINVAL;
  if ((shs != nullptr) == (colors_precomp != nullptr)) return HGS_ESHAPE;
  if ((scales != nullptr) != (rotations != nullptr)) return HGS_ESHAPE;
  if ((scales != nullptr) == (cov3D_precomp != nullptr)) return HGS_ESHAPE;
  if (shs && !dL_dshs) return HGS_EINVAL;
  const bool maybe_entries = status ? status->num_rendered > 0 : entry_capacity > 0;
  if (maybe_entries && (!bin || !bwd_scratch)) return HGS_EINVAL;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  DeviceState* const ds = device_state(stream);
  const int64_t cap = entry_capacity;
  const View v = make_view(s, B, P, M, cap, 0, activation_flags);
  const Layout L = make_layout(const_cast<void*>(geom), const_cast<void*>(bin),
                               const_cast<void*>(img), B, P, v.H, v.W, cap);
  const hgs_status* status_dev = reinterpret_cast<const hgs_status*>(
      static_cast<const char*>(geom) + carve_geom(B, P, v.H, v.W).status);
  // gradient rows: [X entries][12] then the pair rows [pair_cap][10]; X = what the caller sized the scratch by, pair_cap =
  // status->num_pairs (hgs_bwd_scratch_bytes_pairs) or the worst case of 16 per entry (hgs_bwd_scratch_bytes).  The kernels
  // compare pair_cap with the count the sort left on the device: a stale / wrong count writes nothing out of bounds and
  // turns the gradients into NaN instead.
  const int64_t X = status ? (int64_t)status->num_rendered : cap;
  const int64_t worst = X * HGS_PAIRS_PER_ENTRY;
  const int64_t pc = (status && status->num_pairs > 0 && (int64_t)status->num_pairs < worst) ? (int64_t)status->num_pairs : worst;
  const uint32_t pair_cap = (uint32_t)(pc > 0xffffffffll ? 0xffffffffll : pc);
  float* rows = static_cast<float*>(bwd_scratch);
  float* pair_rows = rows + (size_t)X * HGS_ROW_FLOATS;
  HGS_STAGE(0);
  if (maybe_entries) {
    // persistent workgroups of HGS_BWD_BLOCK_WAVES waves: as many waves as the chip holds (LDS: 11.8 KB per wave =>
    // 12 per CU, 3 per SIMD); the waves of a workgroup draw its groups of four work items through an LDS ticket
    const int resident = hgs_knob("HGS_BWD_WAVES_PER_CU", 12) * cu_count(ds);
    hipLaunchKernelGGL(hgs_k_render_bwd, dim3((unsigned)std::max(HGS_NXCD, resident / HGS_BWD_BLOCK_WAVES / HGS_NXCD * HGS_NXCD)), dim3(64 * HGS_BWD_BLOCK_WAVES), 0, stream, v, L, status_dev, L.recs, L.cstate,
                       out_color, out_depth, out_alpha, dL_dout_color, dL_dout_depth, dL_dout_alpha, pair_rows, pair_cap);
    HGS_LAUNCH_CHECK();
    HGS_STAGE(1);
    if (X > 0) {
      // a caller that holds the status hands the reduction its entry count (no status round trip in front of its chain)
      const uint32_t R_host = status ? status->num_rendered : 0xffffffffu;
      hipLaunchKernelGGL(v.pairchunks ? hgs_k_pair_reduce_ch : hgs_k_pair_reduce_em, dim3((unsigned)((X + 255) / 256)), dim3(256), 0,
                         stream, v, L, status_dev, L.recs, pair_rows, rows, pair_cap, R_host);
      HGS_LAUNCH_CHECK();
    }
  }
  if (!maybe_entries) HGS_STAGE(1);
  HGS_STAGE(2);
  // One view: the instantiation without the loop over views (94 instead of 176 VGPRs at SH degree 0).  Several
  // views: one thread per (Gaussian, view) - a workgroup of B waves per 64 Gaussians, summed in view order
  // through LDS (preprocess.hip, mode 2); combinations whose exchange buffer would not fit: the loop.
  const int deg = shs ? v.D : 0;
  const int nc = (deg + 1) * (deg + 1);
  const int aa = (activation_flags & HGS_ANTIALIAS) ? 1 : 0;   // (the filter's copies of the kernels; d3 switches at run time)
  const unsigned thr_p = 64u * (unsigned)v.B;
  const size_t lds_p = (size_t)(23 + 3 * nc) * thr_p * sizeof(float);
  // The exchange buffer may take the CU's whole LDS (160 KB on gfx950; beyond 64 KB the kernel's dynamic-LDS limit is raised
  // first): with the launch bounds of hgs_pre_bwd_forms 16 views at SH degrees 0 / 1, 8 at degrees 2 / 3 (139 KB at degree 3)
  // - the thread-per-(Gaussian, view) form then covers every batch a training step makes; the loop form (d*: 256 VGPRs at
  // degree 3, one wave per SIMD) remains for what does not fit or when the limit cannot be raised.
  const int row_p = hgs_pre_bwd_row(aa, 2, deg);
  const bool vpar_ok = v.B >= HGS_PRE_BWD_VPAR_MIN_VIEWS && thr_p <= (unsigned)hgs_pre_bwd_forms.row[row_p].threads &&
                       (lds_p <= 65536 || pre_bwd_lds_raised(ds, row_p));
  const int mode = v.B == 1 ? 1 : (vpar_ok ? 2 : 0);
  const PreBwdForm& form = hgs_pre_bwd_forms.row[hgs_pre_bwd_row(aa, mode, deg)];
  // s, d: a thread per Gaussian (s at degree >= 1: SH blocks through LDS, <= 53 KB); p: a wave per view of 64 Gaussians
  const unsigned grid = mode == 2 ? (unsigned)((v.P + 63) / 64) : (unsigned)v.nblk, threads = mode == 2 ? thr_p : HGS_BLOCK;
  const size_t lds = mode == 2 ? lds_p : (mode == 1 ? hgs_pre_bwd_stage_bytes(M, deg, shs != nullptr && dL_dshs != nullptr) : 0);
  hipLaunchKernelGGL(form.kernel, dim3(grid), dim3(threads), lds, stream, v, L, status_dev, rows, means3D, shs,
                     colors_precomp, opacities, scales, rotations, cov3D_precomp, dL_dmeans3D, dL_dmeans2D,
                     dL_dshs, dL_dcolors_precomp, dL_dopacities, dL_dscales, dL_drotations,
                     dL_dcov3D_precomp, pack, (int)pack_F);
  HGS_LAUNCH_CHECK();
  HGS_STAGE(3);
  return HGS_OK;
}
}  // namespace

extern "C" {

int hgs_backward_batch_act(const hgs_settings* s, int32_t B, int32_t P, int32_t M, const float* means3D,
                           const float* shs, const float* colors_precomp, const float* opacities,
                           const float* scales, const float* rotations, const float* cov3D_precomp,
                           const int32_t* radii, const float* out_color, const float* out_depth,
                           const float* out_alpha, const float* dL_dout_color,
                           const float* dL_dout_depth, const float* dL_dout_alpha, const void* geom,
                           const void* bin, const void* img, const hgs_status* status,
                           int64_t entry_capacity, void* bwd_scratch, float* dL_dmeans3D, float* dL_dmeans2D, float* dL_dshs,
                           float* dL_dcolors_precomp, float* dL_dopacities, float* dL_dscales,
                           float* dL_drotations, float* dL_dcov3D_precomp, void* const* stage_events,
                           int32_t activation_flags, void* stream_) {
  return backward_impl(s, B, P, M, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, radii, out_color,
                       out_depth, out_alpha, dL_dout_color, dL_dout_depth, dL_dout_alpha, geom, bin, img, status,
                       entry_capacity, bwd_scratch, dL_dmeans3D, dL_dmeans2D, dL_dshs, dL_dcolors_precomp, dL_dopacities,
                       dL_dscales, dL_drotations, dL_dcov3D_precomp, stage_events, activation_flags, nullptr, 0, stream_);
}

int hgs_backward_batch_packed(const hgs_settings* s, int32_t B, int32_t P, int32_t M, const float* means3D,
                              const float* shs, const float* opacities, const float* scales, const float* rotations,
                              const int32_t* radii, const float* out_color, const float* out_depth, const float* out_alpha,
                              const float* dL_dout_color, const float* dL_dout_depth, const float* dL_dout_alpha,
                              const void* geom, const void* bin, const void* img, const hgs_status* status,
                              int64_t entry_capacity, void* bwd_scratch, float* pack, float* dL_dmeans2D_views,
                              void* const* stage_events, int32_t activation_flags, void* stream_) {
  if (!pack || !shs || !scales || !rotations || M < 1) return P == 0 ? HGS_OK : HGS_EINVAL;
  float* marker = pack;        // (non-null markers: the row carries the SH, scale and rotation parts)
  return backward_impl(s, B, P, M, means3D, shs, nullptr, opacities, scales, rotations, nullptr, radii, out_color, out_depth,
                       out_alpha, dL_dout_color, dL_dout_depth, dL_dout_alpha, geom, bin, img, status, entry_capacity,
                       bwd_scratch, marker, dL_dmeans2D_views, marker, nullptr, marker, marker, marker, nullptr, stage_events,
                       activation_flags, pack, 15 + 3 * M, stream_);
}

int hgs_backward_batch(const hgs_settings* s, int32_t B, int32_t P, int32_t M, const float* means3D,
                       const float* shs, const float* colors_precomp, const float* opacities,
                       const float* scales, const float* rotations, const float* cov3D_precomp,
                       const int32_t* radii, const float* out_color, const float* out_depth,
                       const float* out_alpha, const float* dL_dout_color,
                       const float* dL_dout_depth, const float* dL_dout_alpha, const void* geom,
                       const void* bin, const void* img, const hgs_status* status,
                       int64_t entry_capacity, void* bwd_scratch, float* dL_dmeans3D, float* dL_dmeans2D, float* dL_dshs,
                       float* dL_dcolors_precomp, float* dL_dopacities, float* dL_dscales,
                       float* dL_drotations, float* dL_dcov3D_precomp, void* const* stage_events,
                       void* stream_) {
  return hgs_backward_batch_act(s, B, P, M, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                radii, out_color, out_depth, out_alpha, dL_dout_color, dL_dout_depth, dL_dout_alpha,
                                geom, bin, img, status, entry_capacity, bwd_scratch, dL_dmeans3D, dL_dmeans2D, dL_dshs,
                                dL_dcolors_precomp, dL_dopacities, dL_dscales, dL_drotations, dL_dcov3D_precomp,
                                stage_events, 0, stream_);
}

int hgs_backward(const hgs_settings* s, int32_t P, int32_t M, const float* means3D,
                 const float* shs, const float* colors_precomp, const float* opacities,
                 const float* scales, const float* rotations, const float* cov3D_precomp,
                 const int32_t* radii, const float* out_color, const float* out_depth,
                 const float* out_alpha, const float* dL_dout_color,
                 const float* dL_dout_depth, const float* dL_dout_alpha, const void* geom,
                 const void* bin, const void* img, const hgs_status* status,
                 int64_t entry_capacity, void* bwd_scratch, float* dL_dmeans3D, float* dL_dmeans2D, float* dL_dshs,
                 float* dL_dcolors_precomp, float* dL_dopacities, float* dL_dscales,
                 float* dL_drotations, float* dL_dcov3D_precomp, void* const* stage_events,
                 void* stream_) {
  return hgs_backward_batch(s, 1, P, M, means3D, shs, colors_precomp, opacities, scales, rotations,
                            cov3D_precomp, radii, out_color, out_depth, out_alpha, dL_dout_color,
                            dL_dout_depth, dL_dout_alpha, geom, bin, img, status, entry_capacity, bwd_scratch,
                            dL_dmeans3D, dL_dmeans2D, dL_dshs, dL_dcolors_precomp, dL_dopacities, dL_dscales,
                            dL_drotations, dL_dcov3D_precomp, stage_events, stream_);
}

int hgs_densify_stats(int32_t B, int32_t P, const float* dL_dmeans2D, const int32_t* radii, const uint8_t* keep,
                      float* xyz_gradient_accum, float* denom, float* max_radii2D, int32_t* radii_max,
                      uint8_t* visibility, void* stream_) {
  if (B < 1 || P < 0) return HGS_EINVAL;
  if (P == 0) return HGS_OK;
  if (!dL_dmeans2D || !radii || !xyz_gradient_accum || !denom || !max_radii2D) return HGS_EINVAL;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(hgs_k_densify_stats, dim3((P + 255) / 256), dim3(256), 0, stream, (int)B, (int)P, dL_dmeans2D,
                     radii, keep, xyz_gradient_accum, denom, max_radii2D, radii_max, visibility);
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

int hgs_densify_masks(int32_t P, const float* xyz_gradient_accum, const float* denom, const float* scales,
                      int32_t scales_are_log, const float* opacity, int32_t opacity_is_logit,
                      const float* max_radii2D, float grad_threshold, float percent_dense, float extent,
                      float min_opacity, float max_screen_size, float size_thresh, uint8_t* clone_mask,
                      uint8_t* split_mask, uint8_t* prune_mask, uint32_t* counts, void* stream_) {
  if (P < 0) return HGS_EINVAL;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (counts) {
    hipError_t e = hipMemsetAsync(counts, 0, 3 * sizeof(uint32_t), stream);
    if (e != hipSuccess) return hip_rc(e);
  }
  if (P == 0) return HGS_OK;
  if (!xyz_gradient_accum || !denom || !scales || !opacity || (max_screen_size > 0.0f && !max_radii2D)) return HGS_EINVAL;
  hipLaunchKernelGGL(hgs_k_densify_masks, dim3((P + 255) / 256), dim3(256), 0, stream, (int)P, xyz_gradient_accum, denom,
                     scales, (int)scales_are_log, opacity, (int)opacity_is_logit, max_radii2D, grad_threshold,
                     percent_dense, extent, min_opacity, max_screen_size, size_thresh, clone_mask, split_mask, prune_mask,
                     counts);
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

size_t hgs_compact_scratch_bytes(int32_t P) {
  return hgs_align_up(scan_shape((size_t)(P > 0 ? P : 0), 4).bsum_bytes, ALIGN);
}

int hgs_compact_index(int32_t P, const uint8_t* keep, int32_t* src_of_dst, uint32_t* num_kept, void* scratch,
                      void* stream_) {
  if (P < 0 || !num_kept) return HGS_EINVAL;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (P == 0) {
    hipError_t e = hipMemsetAsync(num_kept, 0, 4, stream);
    return e == hipSuccess ? HGS_OK : hip_rc(e);
  }
  if (!keep || !src_of_dst || !scratch) return HGS_EINVAL;
  const int nb = (int)scan_shape((size_t)P, 4).blocks;
  uint32_t* blocks = static_cast<uint32_t*>(scratch);
  hipLaunchKernelGGL(hgs_k_keep_count, dim3(nb), dim3(1024), 0, stream, (int)P, keep, blocks);
  hipLaunchKernelGGL(hgs_k_keep_scan, dim3(1), dim3(1024), 0, stream, nb, blocks, num_kept);
  hipLaunchKernelGGL(hgs_k_keep_index, dim3(nb), dim3(1024), 0, stream, (int)P, keep, blocks, src_of_dst);
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

int hgs_gather_rows(int64_t n_out, int32_t row_floats, const int32_t* src_of_dst, const float* src, float* dst,
                    void* stream_) {
  if (n_out < 0 || row_floats < 1) return HGS_EINVAL;
  if (n_out == 0) return HGS_OK;
  if (!src_of_dst || !src || !dst) return HGS_EINVAL;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const long long n = (long long)n_out * row_floats;
  hipLaunchKernelGGL(hgs_k_gather_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, (int)row_floats,
                     src_of_dst, src, dst);
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

int hgs_reanchor(int32_t P, const float* vertices, const int32_t* faces, const int32_t* mapping_face,
                 const float* mapping_uvw, const float* mapping_dist, float* xyz, void* stream_) {
  if (P < 0) return HGS_EINVAL;
  if (P == 0) return HGS_OK;
  if (!vertices || !faces || !mapping_face || !mapping_uvw || !mapping_dist || !xyz) return HGS_EINVAL;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(hgs_k_reanchor, dim3((P + 255) / 256), dim3(256), 0, stream, (int)P, vertices, faces, mapping_face,
                     mapping_uvw, mapping_dist, xyz);
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

int hgs_reanchor_rot(int32_t P, const float* vertices, const int32_t* faces, const int32_t* mapping_face,
                     const float* mapping_uvw, const float* mapping_dist, const float* rot_in, int32_t bind, float* xyz,
                     float* rot_out, void* stream_) {
  if (P < 0) return HGS_EINVAL;
  if (P == 0) return HGS_OK;
  if (!vertices || !faces || !mapping_face || !mapping_uvw || !mapping_dist || !rot_in || !rot_out) return HGS_EINVAL;
  if (!bind && !xyz) return HGS_EINVAL;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (bind)
    hipLaunchKernelGGL(hgs_k_reanchor_rot_bind, dim3((P + 255) / 256), dim3(256), 0, stream, (int)P, vertices, faces,
                       mapping_face, mapping_uvw, mapping_dist, rot_in, xyz, rot_out);
  else
    hipLaunchKernelGGL(hgs_k_reanchor_rot_pose, dim3((P + 255) / 256), dim3(256), 0, stream, (int)P, vertices, faces,
                       mapping_face, mapping_uvw, mapping_dist, rot_in, xyz, rot_out);
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

// One launch for every tensor of the call (optim.hip): tensor k gets one workgroup per HGS_ADAM_BLOCK_ELEMS elements; beyond
// HGS_ADAM_MAX_BLOCKS in all, every tensor's share shrinks in proportion (at least one) and its workgroups grid-stride.
int hgs_adam_step(const hgs_adam_args* args, void* stream_) {
  if (!args || args->num_tensors < 0 || args->num_tensors > HGS_ADAM_MAX_TENSORS) return HGS_EINVAL;
  hgs_adam_args a = *args;
  if (a.visible && a.visible_rows < 0) return HGS_EINVAL;
  unsigned long long want[HGS_ADAM_MAX_TENSORS], total = 0;
  for (int k = 0; k < a.num_tensors; ++k) {
    const hgs_adam_tensor& t = a.t[k];
    if (t.rows < 0 || t.row_floats < 0) return HGS_EINVAL;
    if (t.row_floats > 0 && (unsigned long long)t.rows > (1ull << 62) / (unsigned long long)t.row_floats) return HGS_EINVAL;
    if (a.visible && t.rows != a.visible_rows) return HGS_ESHAPE;
    const unsigned long long n = (unsigned long long)t.rows * (unsigned long long)t.row_floats;
    if (n > 0 && (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq)) return HGS_EINVAL;
    want[k] = (n + HGS_ADAM_BLOCK_ELEMS - 1) / HGS_ADAM_BLOCK_ELEMS;
    total += want[k];
  }
  if (total == 0) return HGS_OK;
  uint32_t start = 0;
  for (int k = 0; k < a.num_tensors; ++k) {
    a.block_start[k] = start;
    unsigned long long nb = want[k];
    if (total > HGS_ADAM_MAX_BLOCKS && nb > 0) nb = std::max<unsigned long long>(1, nb * HGS_ADAM_MAX_BLOCKS / total);
    start += (uint32_t)nb;
  }
  for (int k = a.num_tensors; k <= HGS_ADAM_MAX_TENSORS; ++k) a.block_start[k] = start;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(hgs_k_adam, dim3(start), dim3(HGS_ADAM_THREADS), 0, stream, a);
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

size_t hgs_lbs_workspace_bytes(int32_t J, int32_t F) {
  if (J < 1 || J > HGS_LBS_MAX_JOINTS || F < 0) return 0;
  return hgs_align_up(((size_t)F * J * 15 + (size_t)F * 9 * (J - 1)) * sizeof(float), 256);
}

// Two launches (lbs.hip): one wave per frame for the joints, then one workgroup per (64 vertices, tile of frames).
int hgs_lbs_pose(const hgs_lbs_args* args, void* stream_) {
  if (!args) return HGS_EINVAL;
  const hgs_lbs_args& a = *args;
  if (a.J < 1 || a.J > HGS_LBS_MAX_JOINTS || a.V < 0 || a.V > (1 << 29) || a.F < 0) return HGS_EINVAL;
  if (a.K != 0 && a.K != 9 * (a.J - 1)) return HGS_EINVAL;
  if (a.weight_width < 1 || a.weight_width > a.J) return HGS_EINVAL;
  if (a.F == 0 || a.V == 0) return HGS_OK;
  if (!a.v_shaped || !a.J_rest || !a.parents || !a.weight_joint || !a.weight_value || !a.poses || !a.workspace || !a.vertices)
    return HGS_EINVAL;
  if (a.K > 0) {
    const long long need = 12ll * ((a.V + 3) / 4);
    if (!a.posedirs || ((uintptr_t)a.posedirs & 15) || (a.posedirs_stride & 3) || a.posedirs_stride < need) return HGS_EINVAL;
  }
  if ((uintptr_t)a.workspace & 15) return HGS_EINVAL;
  const bool one = a.F == 1;
  const unsigned long long tiles = one ? 1ull : ((unsigned long long)a.F + HGS_LBS_FRAME_TILE - 1) / HGS_LBS_FRAME_TILE;
  const unsigned long long blocks = tiles * (unsigned long long)((a.V + HGS_LBS_VERTS - 1) / HGS_LBS_VERTS);
  if (blocks > 0x7fffffffull) return HGS_EINVAL;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(hgs_k_lbs_joints, dim3((unsigned)a.F), dim3(64), 0, stream, a);
  HGS_LAUNCH_CHECK();
  if (one) hipLaunchKernelGGL(hgs_k_lbs_skin_f1, dim3((unsigned)blocks), dim3(HGS_LBS_THREADS), 0, stream, a);
  else hipLaunchKernelGGL(hgs_k_lbs_skin_f8, dim3((unsigned)blocks), dim3(HGS_LBS_THREADS), 0, stream, a);
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

size_t hgs_pose_records_bytes(int32_t style, int32_t B) {
  if ((style != HGS_POSE_OPENPOSE && style != HGS_POSE_HUMANSD) || B < 0) return 0;
  return (size_t)B * hgs_pose_num_records(style) * HGS_POSE_RECORD_INTS * sizeof(int32_t);
}

namespace {
// the styles' own tables, from their public definitions: {colour index, keypoint a, keypoint b}.
// HumanSD: the COCO-17 skeleton in the order MMPose's HumanSD drawing lists it, colours int(255 c) of seaborn's
// hls_palette(16) (hues i / 16 + 0.01 through colorsys.hls_to_rgb(h, .6, .65)).  OpenPose: the 17 limbs of the 18-point
// body model, limb i in colour i of the controlnet_aux list.
const int32_t POSE_LIMBS_HUMANSD[16][3] = {
    {1, 0, 1}, {0, 0, 2}, {3, 1, 3}, {2, 2, 4}, {5, 3, 5}, {4, 4, 6}, {7, 5, 7}, {6, 6, 8},
    {9, 7, 9}, {8, 8, 10}, {11, 5, 11}, {10, 6, 12}, {13, 11, 13}, {12, 12, 14}, {15, 13, 15}, {14, 14, 16}};
const uint8_t POSE_COLOURS_HUMANSD[16][3] = {
    {219, 94, 86}, {219, 144, 86}, {219, 194, 86}, {194, 219, 86}, {145, 219, 86}, {95, 219, 86}, {86, 219, 127}, {86, 219, 177},
    {86, 211, 219}, {86, 161, 219}, {86, 111, 219}, {111, 86, 219}, {160, 86, 219}, {210, 86, 219}, {219, 86, 178}, {219, 86, 128}};
const int32_t POSE_LIMBS_OPENPOSE[17][3] = {
    {0, 0, 1}, {1, 1, 2}, {2, 2, 3}, {3, 3, 4}, {4, 1, 5}, {5, 5, 6}, {6, 6, 7}, {7, 1, 8}, {8, 8, 9},
    {9, 9, 10}, {10, 1, 11}, {11, 11, 12}, {12, 12, 13}, {13, 0, 14}, {14, 14, 16}, {15, 0, 15}, {16, 15, 17}};
const uint8_t POSE_COLOURS_OPENPOSE[18][3] = {
    {255, 0, 0}, {255, 85, 0}, {255, 170, 0}, {255, 255, 0}, {170, 255, 0}, {85, 255, 0}, {0, 255, 0}, {0, 255, 85}, {0, 255, 170},
    {0, 255, 255}, {0, 170, 255}, {0, 85, 255}, {0, 0, 255}, {85, 0, 255}, {170, 0, 255}, {255, 0, 255}, {255, 0, 170}, {255, 0, 85}};
}  // namespace

// One launch (pose.hip): a workgroup per (64 x 16 pixel tile, view).
int hgs_pose_draw(const hgs_pose_args* args, void* stream_) {
  if (!args) return HGS_EINVAL;
  hgs_pose_args a = *args;
  if (a.style != HGS_POSE_OPENPOSE && a.style != HGS_POSE_HUMANSD) return HGS_EINVAL;
  const bool humansd = a.style == HGS_POSE_HUMANSD;
  if (a.K != (humansd ? 17 : 18)) return HGS_EINVAL;
  if (a.B < 0 || a.B > 65535) return HGS_EINVAL;
  if (a.H < 1 || a.H > HGS_POSE_MAX_DIM || a.W < 1 || a.W > HGS_POSE_MAX_DIM) return HGS_EINVAL;
  if (a.limb_width < 1 || a.limb_width > 32767) return HGS_EINVAL;
  const int max_limbs = humansd ? HGS_POSE_MAX_LIMBS - 1 : HGS_POSE_MAX_LIMBS;
  if (a.num_limbs < 0 || a.num_limbs > max_limbs) return HGS_EINVAL;
  if (a.num_limbs == 0) {
    a.num_limbs = max_limbs;
    memset(a.limb, 0, sizeof(a.limb));
    memset(a.colour, 0, sizeof(a.colour));
    if (humansd) { memcpy(a.limb, POSE_LIMBS_HUMANSD, sizeof(POSE_LIMBS_HUMANSD)); memcpy(a.colour, POSE_COLOURS_HUMANSD, sizeof(POSE_COLOURS_HUMANSD)); }
    else { memcpy(a.limb, POSE_LIMBS_OPENPOSE, sizeof(POSE_LIMBS_OPENPOSE)); memcpy(a.colour, POSE_COLOURS_OPENPOSE, sizeof(POSE_COLOURS_OPENPOSE)); }
  } else {
    for (int i = 0; i < a.num_limbs; ++i)
      if (a.limb[i][0] < 0 || a.limb[i][0] >= HGS_POSE_MAX_COLOURS || a.limb[i][1] < 0 || a.limb[i][1] >= a.K ||
          a.limb[i][2] < 0 || a.limb[i][2] >= a.K)
        return HGS_EINVAL;
  }
  if (a.B == 0) return HGS_OK;
  if (!a.points || !a.mvp || !a.image || !a.kp || !a.records) return HGS_EINVAL;
  const unsigned tiles = (unsigned)((a.W + HGS_POSE_TILE_W - 1) / HGS_POSE_TILE_W) * (unsigned)((a.H + HGS_POSE_TILE_H - 1) / HGS_POSE_TILE_H);
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(hgs_k_pose_draw, dim3(tiles, (unsigned)a.B), dim3(HGS_POSE_THREADS), 0, stream, a);
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

namespace {
// sizes both entry points and the workspace rule accept
bool step_images_sizes_ok(int32_t B, int32_t H, int32_t W, int32_t h, int32_t w) {
  if (B < 1 || H < 1 || W < 1 || h < 1 || w < 1 || h > H || w > W) return false;
  if (H > HGS_SI_MAX_DIM || W > HGS_SI_MAX_DIM) return false;
  return (long long)B * H * W <= 0x7fffffffll;
}
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
}  // namespace

size_t hgs_step_images_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t h, int32_t w) {
  if (!step_images_sizes_ok(B, H, W, h, w)) return 0;
  const size_t n = (size_t)B * hgs_si_partials(H, W);
  const size_t fwd = HGS_SI_WS_FWD_WORDS * n, bwd = HGS_SI_WS_BWD_WORDS * n + 2 * (size_t)B + 1;
  return hgs_align_up(std::max(fwd, bwd) * 4, 256);
}

// Three launches (step_images.hip): depth min / max partials; loss partials beside the image planes; one workgroup that
// combines the partials in a fixed order.
int hgs_step_images_forward(const hgs_step_images_args* args, void* stream_) {
  if (!args) return HGS_EINVAL;
  const hgs_step_images_args& a = *args;
  if (!step_images_sizes_ok(a.B, a.H, a.W, a.h, a.w)) return HGS_EINVAL;
  if (!a.render || !a.depth || !a.workspace || !a.rgb_out || !a.depth_out || !a.loss_sparsity || !a.loss_opaque ||
      !a.depth_min || !a.depth_max || !a.depth_global_max || !a.tie_counts)
    return HGS_EINVAL;
  if (!aligned16(a.render) || !aligned16(a.depth) || !aligned16(a.workspace) || !aligned16(a.rgb_out) || !aligned16(a.depth_out))
    return HGS_EINVAL;
  const int P = hgs_si_partials(a.H, a.W);
  const long long per_plane = ((long long)a.h * ((a.w + 3) / 4) + HGS_SI_THREADS - 1) / HGS_SI_THREADS;
  const long long blocks = (long long)a.B * P + 4ll * a.B * per_plane;
  if (blocks > 0x7fffffffll || a.B > 65535) return HGS_EINVAL;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(hgs_k_si_minmax, dim3((unsigned)P, (unsigned)a.B), dim3(HGS_SI_THREADS), 0, stream, a);
  HGS_LAUNCH_CHECK();
  hipLaunchKernelGGL(hgs_k_si_forward, dim3((unsigned)blocks), dim3(HGS_SI_THREADS), 0, stream, a, P, (int)per_plane);
  HGS_LAUNCH_CHECK();
  hipLaunchKernelGGL(hgs_k_si_finish, dim3(1), dim3(HGS_SI_THREADS), 0, stream, a, P);
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

// Three launches: partials of the three tie-share sums; one workgroup that turns them into shares; the two gradients.
// With grad_rgb alone the first two are skipped.
int hgs_step_images_backward(const hgs_step_images_args* args, void* stream_) {
  if (!args) return HGS_EINVAL;
  const hgs_step_images_args& a = *args;
  if (!step_images_sizes_ok(a.B, a.H, a.W, a.h, a.w)) return HGS_EINVAL;
  const bool want_depth = a.grad_depth || a.grad_loss_sparsity || a.grad_loss_opaque;
  if (!a.grad_rgb && !want_depth) return HGS_OK;
  if (a.grad_rgb && (!a.grad_render || !aligned16(a.grad_rgb) || !aligned16(a.grad_render))) return HGS_EINVAL;
  if (want_depth) {
    if (!a.depth || !a.workspace || !a.depth_min || !a.depth_max || !a.depth_global_max || !a.tie_counts || !a.grad_depth_in)
      return HGS_EINVAL;
    if (!aligned16(a.depth) || !aligned16(a.workspace) || !aligned16(a.grad_depth_in) || !aligned16(a.grad_depth)) return HGS_EINVAL;
  }
  const int P = hgs_si_partials(a.H, a.W);
  const int planes = (a.grad_rgb ? 3 : 0) + (want_depth ? 1 : 0);
  const long long per_plane = ((long long)a.H * ((a.W + 3) / 4) + HGS_SI_THREADS - 1) / HGS_SI_THREADS;
  const long long blocks = (long long)planes * a.B * per_plane;
  if (blocks > 0x7fffffffll || a.B > 65535) return HGS_EINVAL;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (want_depth) {
    hipLaunchKernelGGL(hgs_k_si_bwd_sums, dim3((unsigned)P, (unsigned)a.B), dim3(HGS_SI_THREADS), 0, stream, a);
    HGS_LAUNCH_CHECK();
    hipLaunchKernelGGL(hgs_k_si_bwd_finish, dim3(1), dim3(HGS_SI_THREADS), 0, stream, a, P);
    HGS_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(hgs_k_si_bwd_write, dim3((unsigned)blocks), dim3(HGS_SI_THREADS), 0, stream, a, P, (int)per_plane, planes);
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

namespace {
// sizes both entry points and the workspace rule accept
bool photometric_sizes_ok(int32_t B, int32_t C, int32_t H, int32_t W) {
  if (B < 1 || C < 1 || H < 1 || W < 1 || H > HGS_SI_MAX_DIM || W > HGS_SI_MAX_DIM) return false;
  if ((long long)B * C > 65535) return false;
  return (long long)B * C * H * W <= 0x7fffffffll;
}
}  // namespace

size_t hgs_photometric_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t with_grad) {
  if (!photometric_sizes_ok(B, C, H, W)) return 0;
  return pm_carve(B, C, H, W, with_grad).total;
}

// Two launches (photometric.hip): one workgroup per tile of a plane, then one workgroup that adds the partials.
int hgs_photometric_forward(const hgs_photometric_args* args, void* stream_) {
  if (!args) return HGS_EINVAL;
  const hgs_photometric_args& a = *args;
  if (!photometric_sizes_ok(a.B, a.C, a.H, a.W)) return HGS_EINVAL;
  if (!a.image || !a.gt || !a.workspace || !a.loss || !a.l1 || !a.ssim || !a.ssim_image || !a.sqerr || !a.psnr) return HGS_EINVAL;
  const int tiles = pm_tiles(a.H, a.W);
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(hgs_k_pm_forward, dim3((unsigned)tiles, (unsigned)(a.B * a.C)), dim3(HGS_PM_THREADS), 0, stream, a,
                     pm_tiles_x(a.W));
  HGS_LAUNCH_CHECK();
  hipLaunchKernelGGL(hgs_k_pm_finish, dim3(1), dim3(HGS_PM_FINISH_THREADS), 0, stream, a, tiles);
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

// One launch: the three derivative maps of the forward filtered, and the sign term.
int hgs_photometric_backward(const hgs_photometric_args* args, void* stream_) {
  if (!args) return HGS_EINVAL;
  const hgs_photometric_args& a = *args;
  if (!photometric_sizes_ok(a.B, a.C, a.H, a.W)) return HGS_EINVAL;
  if (!a.grad_loss && !a.grad_l1 && !a.grad_ssim && !a.grad_ssim_image) return HGS_OK;
  if (!a.image || !a.gt || !a.workspace || !a.grad_image) return HGS_EINVAL;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(hgs_k_pm_backward, dim3((unsigned)pm_tiles(a.H, a.W), (unsigned)(a.B * a.C)), dim3(HGS_PM_THREADS), 0, stream, a,
                     pm_tiles_x(a.W));
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

namespace {
struct MeshCarve { size_t tris, start, cursor, bsum, refs, total; };
MeshCarve carve_mesh(int32_t F, uint32_t ncells, uint64_t nrefs) {
  MeshCarve c;
  Carver cv;
  cv.take(sizeof(MeshGridHdr));
  c.tris = cv.take((size_t)F * 48);
  c.start = cv.take(((size_t)ncells + 1) * 4);
  c.cursor = cv.take((size_t)ncells * 4);
  c.bsum = cv.take(scan_shape((size_t)ncells + 1, 4).bsum_bytes);          // (sized like start[]: with the end sentinel)
  c.refs = cv.take((size_t)nrefs * 4);
  c.total = cv.off;
  return c;
}
bool mesh_info_ok(const hgs_mesh_grid_info* in) {
  if (!in || in->num_faces < 1 || in->num_refs > 0x7fffffffull || !(in->cell > 0.0f)) return false;
  unsigned long long n = 1;
  for (int a = 0; a < 3; ++a) {
    if (in->dims[a] < 1 || in->dims[a] > 4096) return false;
    n *= (unsigned long long)in->dims[a];
  }
  return n == in->ncells && n <= HGS_MESH_MAX_CELLS;
}
}  // namespace

int hgs_mesh_grid_plan(int32_t V, const float* vertices, int32_t F, const int32_t* faces, hgs_mesh_grid_info* info,
                       void* stream_) {
  if (V < 0 || F < 1 || !info || !faces || (V > 0 && !vertices)) return HGS_EINVAL;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const hipError_t e = box_init(info, sizeof(hgs_mesh_grid_info), info->bmin, stream);
  if (e != hipSuccess) return hip_rc(e);
  if (V > 0) hipLaunchKernelGGL(hgs_k_mesh_bbox, dim3((V + 255) / 256), dim3(256), 0, stream, (int)V, vertices, info);
  hipLaunchKernelGGL(hgs_k_mesh_grid_setup, dim3(1), dim3(64), 0, stream, (int)F, info);
  hipLaunchKernelGGL(hgs_k_mesh_count_refs, dim3((F + 255) / 256), dim3(256), 0, stream, (int)V, vertices, (int)F, faces, info);
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

size_t hgs_mesh_grid_bytes(const hgs_mesh_grid_info* info_host) {
  if (!mesh_info_ok(info_host)) return 0;
  return carve_mesh(info_host->num_faces, info_host->ncells, info_host->num_refs).total;
}

int hgs_mesh_grid_build(int32_t V, const float* vertices, int32_t F, const int32_t* faces,
                        const hgs_mesh_grid_info* info_host, void* grid, void* stream_) {
  if (V < 0 || F < 1 || !faces || !grid || (V > 0 && !vertices) || !mesh_info_ok(info_host) || info_host->num_faces != F)
    return HGS_EINVAL;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const hgs_mesh_grid_info& in = *info_host;
  const MeshCarve c = carve_mesh(F, in.ncells, in.num_refs);
  MeshGridHdr G;
  G.gx = in.dims[0]; G.gy = in.dims[1]; G.gz = in.dims[2];
  G.ncells = in.ncells;
  G.ox = in.origin[0]; G.oy = in.origin[1]; G.oz = in.origin[2];
  G.h = in.cell;
  G.inv_h = 1.0f / in.cell;            // (the plan's count_refs divides the same way)
  G.cmax = 0.0f;
  for (int a = 0; a < 3; ++a)
    G.cmax = std::max(G.cmax, std::max(fabsf(in.origin[a]), fabsf(in.origin[a] + (float)in.dims[a] * in.cell)));
  G.F = F;
  G.nrefs = (uint32_t)in.num_refs;
  G.off_tris = c.tris; G.off_start = c.start; G.off_cursor = c.cursor; G.off_bsum = c.bsum; G.off_refs = c.refs;
  const unsigned long long n_init = std::max<unsigned long long>((unsigned long long)in.ncells + 1, (unsigned long long)F);
  const unsigned gf = (unsigned)((F + 255) / 256), gc = scan_shape(in.ncells, 4).blocks;
  hipLaunchKernelGGL(hgs_k_mesh_grid_init, dim3((unsigned)((n_init + 255) / 256)), dim3(256), 0, stream, G, (int)V,
                     vertices, faces, grid);
  hipLaunchKernelGGL(hgs_k_mesh_bin, dim3(gf), dim3(256), 0, stream, G, grid, 0);
  hipLaunchKernelGGL(hgs_k_mesh_scan1, dim3(gc), dim3(1024), 0, stream, G, grid);
  hipLaunchKernelGGL(hgs_k_mesh_scan2, dim3(1), dim3(1024), 0, stream, G, grid);
  hipLaunchKernelGGL(hgs_k_mesh_scan3, dim3(gc), dim3(1024), 0, stream, G, grid);
  hipLaunchKernelGGL(hgs_k_mesh_bin, dim3(gf), dim3(256), 0, stream, G, grid, 1);
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

int hgs_mesh_query(int32_t P, const float* points, int32_t V, const float* vertices, int32_t F, const int32_t* faces,
                   const void* grid, int32_t mode, float* dist, int32_t* face, float* uvw, void* stream_) {
  if (P < 0 || V < 0 || F < 0 || (mode != HGS_MESH_UNSIGNED && mode != HGS_MESH_RAYSTAB)) return HGS_EINVAL;
  if (P == 0) return HGS_OK;
  if (F == 0 || !points || !dist || !face) return HGS_EINVAL;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const unsigned gp = (unsigned)((P + 255) / 256);
  if (grid) {
    hipLaunchKernelGGL(hgs_k_mesh_query_grid, dim3(gp), dim3(256), 0, stream, (int)P, points, grid, (int)mode, dist, face, uvw);
  } else {
    if (!faces || (V > 0 && !vertices)) return HGS_EINVAL;
    hipLaunchKernelGGL(hgs_k_mesh_query_brute, dim3(gp), dim3(256), 0, stream, (int)P, points, (int)V, vertices, (int)F,
                       faces, (int)mode, dist, face, uvw);
  }
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

namespace {
struct FieldPlanCarve { size_t rec, reach, bounds, counts, total; };
FieldPlanCarve carve_field_plan(int32_t P, int32_t nb) {
  FieldPlanCarve c;
  Carver cv;
  c.rec = cv.take((size_t)P * HGS_FIELD_REC_FLOATS * 4);
  c.reach = cv.take((size_t)P * 4);
  c.bounds = cv.take(2 * HGS_FIELD_MAX_BLOCKS * 4);
  c.counts = cv.take((size_t)nb * nb * nb * 4);
  c.total = cv.off;
  return c;
}
struct FieldListCarve { size_t start, order, refs, total; };
FieldListCarve carve_field_lists(int32_t nb, uint64_t nrefs) {
  FieldListCarve c;
  Carver cv;
  const size_t nblocks = (size_t)nb * nb * nb;
  c.start = cv.take((nblocks + 1) * 4);
  c.order = cv.take(nblocks * 4);
  c.refs = cv.take((size_t)nrefs * 4);
  c.total = cv.off;
  return c;
}
bool field_dims_ok(int32_t P, int32_t R, int32_t nb) {
  return P >= 0 && nb >= 1 && nb <= HGS_FIELD_MAX_BLOCKS && R >= nb && R <= HGS_FIELD_MAX_RES && R % nb == 0 &&
         R / nb <= HGS_FIELD_MAX_SPLIT;
}
bool field_info_ok(const hgs_field_info* in) {
  return in && field_dims_ok(in->num_gaussians, in->resolution, in->num_blocks) && in->num_refs <= 0x7fffffffull &&
         in->num_kept <= (uint32_t)in->num_gaussians;
}
FieldPlanPtrs field_plan_ptrs(const FieldPlanCarve& c, void* plan) {
  char* b = static_cast<char*>(plan);
  FieldPlanPtrs p;
  p.rec = reinterpret_cast<float2*>(b + c.rec);
  p.reach = reinterpret_cast<uint32_t*>(b + c.reach);
  p.bounds = reinterpret_cast<float*>(b + c.bounds);
  p.counts = reinterpret_cast<uint32_t*>(b + c.counts);
  return p;
}
struct McCarve { size_t offs, bsum, mask, total; };
bool mc_dims_ok(int32_t X, int32_t Y, int32_t Z) {
  if (X < 1 || Y < 1 || Z < 1) return false;
  const unsigned long long xy = (unsigned long long)X * (unsigned long long)Y;      // < 2^62: cannot wrap
  return xy <= (1ull << 28) && xy * (unsigned long long)Z <= (1ull << 28);
}
McCarve carve_mc(size_t N) {
  McCarve c;
  Carver cv;
  c.offs = cv.take((N + 1) * 8);
  c.bsum = cv.take(scan_shape(N, 8).bsum_bytes);
  c.mask = cv.take(N);
  c.total = cv.off;
  return c;
}
McPtrs mc_ptrs(const McCarve& c, void* scratch) {
  char* b = static_cast<char*>(scratch);
  McPtrs p;
  p.offs = reinterpret_cast<uint2*>(b + c.offs);
  p.bsum = reinterpret_cast<uint2*>(b + c.bsum);
  p.mask = reinterpret_cast<uint8_t*>(b + c.mask);
  return p;
}
}  // namespace

size_t hgs_field_plan_bytes(int32_t P, int32_t num_blocks) {
  if (P < 0 || num_blocks < 1 || num_blocks > HGS_FIELD_MAX_BLOCKS) return 0;
  return carve_field_plan(P, num_blocks).total;
}

int hgs_field_plan(int32_t P, const float* xyz, const float* opacity, const float* scaling, const float* rotation,
                   int32_t resolution, int32_t num_blocks, const float* axis, float grow, void* plan,
                   hgs_field_info* info, void* stream_) {
  if (!field_dims_ok(P, resolution, num_blocks) || !axis || !plan || !info || !(grow >= 0.0f)) return HGS_EINVAL;
  if (P > 0 && (!xyz || !opacity || !scaling || !rotation)) return HGS_EINVAL;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const FieldPlanCarve c = carve_field_plan(P, num_blocks);
  const FieldPlanPtrs pp = field_plan_ptrs(c, plan);
  const FieldDims D = {P, resolution, num_blocks, resolution / num_blocks};
  const uint32_t nblocks = (uint32_t)(num_blocks * num_blocks * num_blocks);
  hipError_t e = box_init(info, sizeof(hgs_field_info), info->bmin, stream);
  if (e == hipSuccess) e = hipMemsetAsync(pp.counts, 0, (size_t)nblocks * 4, stream);
  if (e != hipSuccess) return hip_rc(e);
  const unsigned gp = (unsigned)((P + 255) / 256);
  if (P > 0) hipLaunchKernelGGL(hgs_k_field_bbox, dim3(gp), dim3(256), 0, stream, (int)P, xyz, opacity, info);
  hipLaunchKernelGGL(hgs_k_field_setup, dim3(1), dim3(64), 0, stream, D, axis, grow, pp, info);
  if (P > 0) {
    hipLaunchKernelGGL(hgs_k_field_gauss, dim3(gp), dim3(256), 0, stream, D, xyz, opacity, scaling, rotation, pp, info);
    hipLaunchKernelGGL(hgs_k_field_lists, dim3((nblocks + 3u) / 4u), dim3(256), 0, stream, D, pp, FieldListPtrs{nullptr, nullptr, nullptr}, 0, info);
  }
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

size_t hgs_field_list_bytes(const hgs_field_info* info_host) {
  if (!field_info_ok(info_host)) return 0;
  return carve_field_lists(info_host->num_blocks, info_host->num_refs).total;
}

int hgs_field_eval(const hgs_field_info* info_host, const float* axis, const void* plan, void* lists, float* occ,
                   int32_t* block_counts, void* stream_) {
  if (!field_info_ok(info_host) || !axis || !plan || !lists || !occ) return HGS_EINVAL;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const hgs_field_info& in = *info_host;
  const FieldDims D = {in.num_gaussians, in.resolution, in.num_blocks, in.resolution / in.num_blocks};
  const FieldPlanPtrs pp = field_plan_ptrs(carve_field_plan(D.P, D.nb), const_cast<void*>(plan));
  const FieldListCarve lc = carve_field_lists(D.nb, in.num_refs);
  char* lb = static_cast<char*>(lists);
  const FieldListPtrs lp = {reinterpret_cast<uint32_t*>(lb + lc.start), reinterpret_cast<uint32_t*>(lb + lc.order),
                            reinterpret_cast<uint32_t*>(lb + lc.refs)};
  const uint32_t nblocks = (uint32_t)(D.nb * D.nb * D.nb);
  hipLaunchKernelGGL(hgs_k_field_order, dim3(1), dim3(1024), 0, stream, D, pp, lp);
  if (in.num_refs > 0)
    hipLaunchKernelGGL(hgs_k_field_lists, dim3((nblocks + 3u) / 4u), dim3(256), 0, stream, D, pp, lp, 1, (hgs_field_info*)nullptr);
  const int items = ((D.split + 1) / 2) * D.split * D.split;
  const int threads = items <= 64 ? 64 : 256;
  const int slabs = (items + threads - 1) / threads;
  hipLaunchKernelGGL(hgs_k_field_eval, dim3(nblocks * (unsigned)slabs), dim3(threads), 0, stream, D, axis, pp, lp, slabs, occ);
  HGS_LAUNCH_CHECK();
  if (block_counts) {
    const hipError_t e = hipMemcpyAsync(block_counts, pp.counts, (size_t)nblocks * 4, hipMemcpyDeviceToDevice, stream);
    if (e != hipSuccess) return hip_rc(e);
  }
  return HGS_OK;
}

namespace {
// scratch of hgs_fsample: the table and the cursors first, as one piece (zeroed by one memset)
struct FSampleCarve { size_t zeroed, zeroed_bytes, blk, bins, total; };
FSampleCarve carve_fsample(int32_t M, int32_t nb) {
  FSampleCarve c;
  Carver cv;
  const size_t nblocks = (size_t)nb * nb * nb;
  c.zeroed_bytes = (nblocks + 1) * 8 + nblocks * 4;
  c.zeroed = cv.take(c.zeroed_bytes);
  c.blk = cv.take((size_t)M * 4);
  c.bins = cv.take((size_t)M * 4);
  c.total = cv.off;
  return c;
}
}  // namespace

size_t hgs_fsample_scratch_bytes(int32_t M, int32_t num_blocks) {
  if (M < 0 || num_blocks < 1 || num_blocks > HGS_FIELD_MAX_BLOCKS) return 0;
  return carve_fsample(M, num_blocks).total;
}

int hgs_fsample(const hgs_fsample_args* args, void* stream_) {
  if (!args) return HGS_EINVAL;
  const hgs_fsample_args& a = *args;
  if (!field_info_ok(a.info_host) || a.M < 0 || (a.color && !a.colors)) return HGS_EINVAL;
  if (a.M == 0 || (!a.density && !a.normal && !a.color)) return HGS_OK;
  if (!a.points) return HGS_EINVAL;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const hgs_field_info& in = *a.info_host;
  const size_t M = (size_t)a.M;
  if (in.num_refs == 0) {                                   // every list is empty (and `lists` need not exist): zeros
    hipError_t e = hipSuccess;
    if (a.density) e = hipMemsetAsync(a.density, 0, M * 4, stream);
    if (e == hipSuccess && a.normal) e = hipMemsetAsync(a.normal, 0, M * 12, stream);
    if (e == hipSuccess && a.color) e = hipMemsetAsync(a.color, 0, M * 12, stream);
    return hip_rc(e);
  }
  if (!a.axis || !a.plan || !a.lists || !a.scratch) return HGS_EINVAL;
  const FieldDims D = {in.num_gaussians, in.resolution, in.num_blocks, in.resolution / in.num_blocks};
  const FieldPlanPtrs pp = field_plan_ptrs(carve_field_plan(D.P, D.nb), const_cast<void*>(a.plan));
  const FieldListCarve lc = carve_field_lists(D.nb, in.num_refs);
  char* lb = static_cast<char*>(const_cast<void*>(a.lists));
  const FieldListPtrs lp = {reinterpret_cast<uint32_t*>(lb + lc.start), reinterpret_cast<uint32_t*>(lb + lc.order),
                            reinterpret_cast<uint32_t*>(lb + lc.refs)};
  const uint32_t nblocks = (uint32_t)(D.nb * D.nb * D.nb);
  const FSampleCarve sc = carve_fsample(a.M, D.nb);
  char* sb = static_cast<char*>(a.scratch);
  FSamplePtrs sp;
  sp.tab = reinterpret_cast<uint2*>(sb + sc.zeroed);
  sp.cursor = reinterpret_cast<uint32_t*>(sb + sc.zeroed + ((size_t)nblocks + 1) * 8);
  sp.blk = reinterpret_cast<uint32_t*>(sb + sc.blk);
  sp.bins = reinterpret_cast<uint32_t*>(sb + sc.bins);
  const FSampleGeo geo = {in.center[0], in.center[1], in.center[2], in.scale, a.normalized ? 1 : 0};
  const FSampleOut out = {a.density, a.normal, a.color};
  const hipError_t e = hipMemsetAsync(sb + sc.zeroed, 0, sc.zeroed_bytes, stream);
  if (e != hipSuccess) return hip_rc(e);
  const unsigned gm = (unsigned)((M + 255) / 256);
  hipLaunchKernelGGL(hgs_k_fsample_bin, dim3(gm), dim3(256), 0, stream, D, (uint32_t)M, a.points, a.axis, geo, sp, out);
  hipLaunchKernelGGL(hgs_k_fsample_table, dim3(1), dim3(1024), 0, stream, D, sp);
  hipLaunchKernelGGL(hgs_k_fsample_scatter, dim3(gm), dim3(256), 0, stream, (uint32_t)M, sp);
  // every block with points has at most one run that is not full: ceil(M / 256) + min(blocks, M) bounds the runs
  const unsigned runs = gm + (unsigned)std::min<size_t>(nblocks, M);
  hipLaunchKernelGGL(hgs_k_fsample_eval, dim3(runs), dim3(HGS_FSAMPLE_RUN), 0, stream, D, a.points, a.colors, geo, pp, lp, sp, out);
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

size_t hgs_mc_scratch_bytes(int32_t X, int32_t Y, int32_t Z) {
  if (!mc_dims_ok(X, Y, Z)) return 0;
  return carve_mc((size_t)X * Y * Z).total;
}

int hgs_mc_count(const float* field, int32_t X, int32_t Y, int32_t Z, float threshold, void* scratch, hgs_mc_info* info,
                 void* stream_) {
  if (!mc_dims_ok(X, Y, Z) || !field || !scratch || !info) return HGS_EINVAL;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const McDims D = {X, Y, Z, (uint32_t)((size_t)X * Y * Z)};
  const McPtrs p = mc_ptrs(carve_mc(D.N), scratch);
  const unsigned g1k = scan_shape(D.N, 8).blocks;
  hipLaunchKernelGGL(hgs_k_mc_count, dim3((D.N + 255u) / 256u), dim3(256), 0, stream, D, field, threshold, p);
  hipLaunchKernelGGL(hgs_k_mc_scan1, dim3(g1k), dim3(1024), 0, stream, D, p);
  hipLaunchKernelGGL(hgs_k_mc_scan2, dim3(1), dim3(1024), 0, stream, D, p, info);
  hipLaunchKernelGGL(hgs_k_mc_scan3, dim3(g1k), dim3(1024), 0, stream, D, p);
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

int hgs_mc_emit(const float* field, int32_t X, int32_t Y, int32_t Z, float threshold, const void* scratch,
                const hgs_mc_info* info_host, float* vertices, int32_t* triangles, void* stream_) {
  if (!mc_dims_ok(X, Y, Z) || !field || !scratch || !info_host) return HGS_EINVAL;
  const uint32_t nv = info_host->num_vertices, nt = info_host->num_triangles;
  const McDims D = {X, Y, Z, (uint32_t)((size_t)X * Y * Z)};
  if (nv > 3ull * D.N || nt > 5ull * D.N || (nv && !vertices) || (nt && !triangles)) return HGS_EINVAL;
  if (nv == 0 && nt == 0) return HGS_OK;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const McPtrs p = mc_ptrs(carve_mc(D.N), const_cast<void*>(scratch));
  hipLaunchKernelGGL(hgs_k_mc_emit, dim3((D.N + 255u) / 256u), dim3(256), 0, stream, D, field, threshold, p, nv, nt, vertices,
                     triangles);
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

int hgs_mark_visible(const hgs_settings* s, int32_t P, const float* means3D, uint8_t* present,
                     void* stream_) {
  if (!s || !s->viewmatrix || P < 0) return HGS_EINVAL;
  if (P == 0) return HGS_OK;
  if (!means3D || !present) return HGS_EINVAL;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(hgs_k_mark_visible, dim3((P + HGS_BLOCK - 1) / HGS_BLOCK), dim3(HGS_BLOCK),
                     0, stream, s->viewmatrix, (int)P, means3D, present);
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

// ---- surface samples and the initial Gaussians (surface.hip) ------------------------------------------------------------
size_t hgs_surface_cdf_scratch_bytes(int32_t F) {
  if (F < 1 || F > HGS_SURFACE_MAX_FACES) return 0;
  return hgs_align_up(scan_shape((size_t)F + 1, 8).bsum_bytes, ALIGN);
}

int hgs_surface_cdf(int32_t V, const float* vertices, int32_t F, const int32_t* faces, double* cdf, hgs_surface_info* info,
                    void* scratch, void* stream_) {
  static_assert(sizeof(hgs_surface_info) == 16 && sizeof(SurfInfo) == 16, "the info block is 16 bytes");
  if (V < 0 || F < 1 || F > HGS_SURFACE_MAX_FACES || !faces || !cdf || !info || !scratch || (V > 0 && !vertices)) return HGS_EINVAL;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const hipError_t e = hipMemsetAsync(info, 0, sizeof(hgs_surface_info), stream);
  if (e != hipSuccess) return hip_rc(e);
  // (F + 1 <= 2^20 entries: at most 1024 blocks, so the carry is ONE left-to-right round over their totals)
  const unsigned nb = scan_shape((size_t)F + 1, 8).blocks;
  double* bsum = static_cast<double*>(scratch);
  hipLaunchKernelGGL(hgs_k_surface_area, dim3(nb), dim3(HGS_SCAN_BLOCK), 0, stream, (int)V, (uint32_t)F, vertices, faces, cdf, bsum);
  hipLaunchKernelGGL(hgs_k_surface_carry, dim3(1), dim3(HGS_SCAN_BLOCK), 0, stream, (uint32_t)nb, bsum);
  hipLaunchKernelGGL(hgs_k_surface_prefix, dim3(nb), dim3(HGS_SCAN_BLOCK), 0, stream, (uint32_t)F, cdf, (const double*)bsum,
                     reinterpret_cast<SurfInfo*>(info));
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

int hgs_surface_sample(const hgs_surface_sample_args* args, void* stream_) {
  if (!args) return HGS_EINVAL;
  const hgs_surface_sample_args& a = *args;
  if (a.N < 0 || a.V < 0 || a.F < 1 || a.F > HGS_SURFACE_MAX_FACES || !a.faces || !a.cdf || (a.V > 0 && !a.vertices))
    return HGS_EINVAL;
  if (a.N == 0 || (!a.points && !a.face && !a.uvw)) return HGS_OK;
  if ((uint64_t)a.N > 0xffffffffull * HGS_SURF_THREADS) return HGS_EINVAL;
  SurfSampleArgs k;
  k.V = a.V; k.F = a.F;
  // every 2^shift-th entry of the table goes to LDS: the smallest shift >= 4 that fits the staging array
  k.shift = 4;
  while ((((size_t)a.F + 1) + ((size_t)1 << k.shift) - 1) >> k.shift > HGS_SURF_COARSE_MAX) ++k.shift;
  k.ncoarse = (int32_t)((((size_t)a.F + 1) + ((size_t)1 << k.shift) - 1) >> k.shift);
  k.vtx = a.vertices; k.faces = a.faces; k.cdf = a.cdf;
  k.N = (unsigned long long)a.N; k.offset = a.offset;
  k.seed_lo = (uint32_t)a.seed; k.seed_hi = (uint32_t)(a.seed >> 32);
  k.points = a.points; k.face = a.face; k.uvw = a.uvw;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(hgs_k_surface_sample, dim3((unsigned)((k.N + HGS_SURF_THREADS - 1) / HGS_SURF_THREADS)),
                     dim3(HGS_SURF_THREADS), 0, stream, k);
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

int hgs_init_gaussians(int64_t P, int32_t M, const float* colors, const float* dist2, float* features_dc,
                       float* features_rest, float* scaling, float* rotation, float* opacity, float* max_radii2D,
                       void* stream_) {
  if (P < 0 || M < 1 || M > 4096) return HGS_EINVAL;
  if (P == 0) return HGS_OK;
  if (scaling && !dist2) return HGS_EINVAL;
  InitGaussiansArgs k;
  k.P = P;
  k.rest_floats = 3 * (M - 1);
  const float q = 0.1f / (1.0f - 0.1f);
  k.opacity = (float)log((double)q);
  k.colors = colors; k.dist2 = dist2;
  k.features_dc = features_dc; k.features_rest = M > 1 ? features_rest : nullptr; k.scaling = scaling; k.rotation = rotation;
  k.opacity_out = opacity; k.max_radii2D = max_radii2D;
  const long long n = (long long)P * (12 + k.rest_floats);
  if ((n + 255) / 256 > 0x7fffffffll) return HGS_EINVAL;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(hgs_k_init_gaussians, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, k);
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

namespace {
struct MvShape { int tiles_x, tiles_y; uint32_t ntiles, n; };
// the sizes the mesh view's calls accept (include/hgs_rast.h)
bool mv_shape(int32_t B, int32_t V, int32_t F, int32_t H, int32_t W, MvShape& s) {
  if (B < 0 || B > 65535 || V < 0 || F < 0 || F > (1 << 24) - 1) return false;
  if (H < 1 || H > HGS_MESHVIEW_MAX_DIM || W < 1 || W > HGS_MESHVIEW_MAX_DIM) return false;
  s.tiles_x = (W + HGS_MESHVIEW_TILE - 1) / HGS_MESHVIEW_TILE;
  s.tiles_y = (H + HGS_MESHVIEW_TILE - 1) / HGS_MESHVIEW_TILE;
  s.ntiles = (uint32_t)(s.tiles_x * s.tiles_y);
  const long long lim = 0x7fffffffll;
  if ((long long)B * V >= lim || (long long)B * F >= lim || (long long)B * s.ntiles >= lim) return false;
  s.n = (uint32_t)B * s.ntiles;
  return true;
}
struct MvCarve { size_t tribox, start, cursor, bsum, total; };
MvCarve carve_mv(int32_t B, int32_t F, const MvShape& s) {
  MvCarve c;
  Carver cv;
  c.tribox = cv.take((size_t)B * F * 4);
  c.start = cv.take(((size_t)s.n + 1) * 4);
  c.cursor = cv.take((size_t)s.n * 4);
  c.bsum = cv.take(scan_shape((size_t)s.n + 1, 4).bsum_bytes);
  c.total = cv.off;
  return c;
}
MvPlanPtrs mv_ptrs(const MvCarve& c, void* plan) {
  char* b = static_cast<char*>(plan);
  return {reinterpret_cast<uint32_t*>(b + c.tribox), reinterpret_cast<uint32_t*>(b + c.start),
          reinterpret_cast<uint32_t*>(b + c.cursor), reinterpret_cast<uint32_t*>(b + c.bsum)};
}
bool mv_strides_ok(const hgs_meshview_args& a) {
  return a.vertex_stride == 0 || a.vertex_stride == 3ll * a.V;
}
bool mv_attr_ok(const hgs_meshview_args& a) {
  if (a.C < 1 || a.C > HGS_MESHVIEW_MAX_ATTR || !a.attr) return false;
  if (a.attr_stride != 0 && a.attr_stride != (long long)a.V * a.C) return false;
  return !a.shade_normals || a.C == 3;
}
}  // namespace

size_t hgs_meshview_plan_bytes(int32_t B, int32_t F, int32_t H, int32_t W) {
  MvShape s;
  if (!mv_shape(B, 0, F, H, W, s)) return 0;
  return carve_mv(B, F, s).total;
}

// One launch (meshview.hip): a thread per (mesh, vertex).
int hgs_meshview_normals(const hgs_meshview_args* args, void* stream_) {
  if (!args) return HGS_EINVAL;
  const hgs_meshview_args& a = *args;
  MvShape s;
  if (!mv_shape(a.B, a.V, a.F, 1, 1, s) || !mv_strides_ok(a)) return HGS_EINVAL;
  const int Bv = a.vertex_stride ? a.B : 1;
  if (a.B == 0 || a.V == 0) return HGS_OK;
  if (!a.vertices || !a.normals || !a.adj_start || (a.F > 0 && (!a.faces || !a.adj))) return HGS_EINVAL;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const long long n = (long long)Bv * a.V;
  hipLaunchKernelGGL(hgs_k_mv_normals, dim3((unsigned)((n + HGS_MV_THREADS - 1) / HGS_MV_THREADS)), dim3(HGS_MV_THREADS), 0,
                     stream, a, Bv);
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

// Two memsets and five launches: vertex records, the triangles' tile boxes and the tiles' counts, the scan.
int hgs_meshview_plan(const hgs_meshview_args* args, void* stream_) {
  if (!args) return HGS_EINVAL;
  const hgs_meshview_args& a = *args;
  MvShape s;
  if (!mv_shape(a.B, a.V, a.F, a.H, a.W, s) || !mv_strides_ok(a)) return HGS_EINVAL;
  if (a.B == 0) return HGS_OK;
  if (!a.mvp || !a.plan || !a.info || (a.V > 0 && (!a.vertices || !a.records)) || (a.F > 0 && !a.faces)) return HGS_EINVAL;
  if (((uintptr_t)a.records & 15) || ((uintptr_t)a.plan & 15) || ((uintptr_t)a.info & 7)) return HGS_EINVAL;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const MvCarve c = carve_mv(a.B, a.F, s);
  const MvPlanPtrs pp = mv_ptrs(c, a.plan);
  hipError_t e = hipMemsetAsync(a.info, 0, sizeof(hgs_meshview_info), stream);
  if (e == hipSuccess) e = hipMemsetAsync(pp.start, 0, ((size_t)s.n + 1) * 4, stream);
  if (e != hipSuccess) return hip_rc(e);
  const long long nv = (long long)a.B * a.V, nf = (long long)a.B * a.F;
  if (nv > 0)
    hipLaunchKernelGGL(hgs_k_mv_vertex, dim3((unsigned)((nv + HGS_MV_THREADS - 1) / HGS_MV_THREADS)), dim3(HGS_MV_THREADS), 0,
                       stream, a);
  if (nf > 0)
    hipLaunchKernelGGL(hgs_k_mv_count, dim3((unsigned)((nf + HGS_MV_THREADS - 1) / HGS_MV_THREADS)), dim3(HGS_MV_THREADS), 0,
                       stream, a, pp, s.tiles_x, s.ntiles);
  const unsigned gs = scan_shape(s.n, 4).blocks;
  hipLaunchKernelGGL(hgs_k_mv_scan1, dim3(gs), dim3(1024), 0, stream, pp, s.n);
  hipLaunchKernelGGL(hgs_k_mv_scan2, dim3(1), dim3(1024), 0, stream, pp, s.n);
  hipLaunchKernelGGL(hgs_k_mv_scan3, dim3(gs), dim3(1024), 0, stream, a, pp, s.n);
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

size_t hgs_meshview_list_bytes(const hgs_meshview_info* info_host) {
  if (!info_host || info_host->num_refs > 0x7fffffffull) return (size_t)-1;
  return hgs_align_up((size_t)info_host->num_refs * 4, ALIGN);
}

// Two launches: the tiles' lists, then one workgroup per tile.
int hgs_meshview_draw(const hgs_meshview_args* args, const hgs_meshview_info* info_host, void* stream_) {
  if (!args || !info_host) return HGS_EINVAL;
  const hgs_meshview_args& a = *args;
  const hgs_meshview_info& in = *info_host;
  MvShape s;
  if (!mv_shape(a.B, a.V, a.F, a.H, a.W, s)) return HGS_EINVAL;
  if (a.B == 0) return HGS_OK;
  if (in.B != a.B || in.V != a.V || in.F != a.F || in.H != a.H || in.W != a.W || in.num_refs > 0x7fffffffull) return HGS_EINVAL;
  if (!a.plan || (!a.rast && !a.image) || (in.num_refs > 0 && (!a.lists || !a.records || !a.faces))) return HGS_EINVAL;
  if (a.image && !mv_attr_ok(a)) return HGS_EINVAL;
  if (((uintptr_t)a.records & 15) || ((uintptr_t)a.plan & 15) || ((uintptr_t)a.rast & 15)) return HGS_EINVAL;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const MvPlanPtrs pp = mv_ptrs(carve_mv(a.B, a.F, s), a.plan);
  const uint32_t nrefs = (uint32_t)in.num_refs;
  const long long nf = (long long)a.B * a.F;
  if (nrefs > 0)
    hipLaunchKernelGGL(hgs_k_mv_fill, dim3((unsigned)((nf + HGS_MV_THREADS - 1) / HGS_MV_THREADS)), dim3(HGS_MV_THREADS), 0,
                       stream, a, pp, s.tiles_x, s.ntiles, nrefs);
  hipLaunchKernelGGL(hgs_k_mv_draw, dim3(s.ntiles, (unsigned)a.B), dim3(HGS_MV_THREADS), 0, stream, a, pp, s.tiles_x, s.ntiles,
                     nrefs);
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

int hgs_meshview_interpolate(const hgs_meshview_args* args, void* stream_) {
  if (!args) return HGS_EINVAL;
  const hgs_meshview_args& a = *args;
  MvShape s;
  if (!mv_shape(a.B, a.V, a.F, a.H, a.W, s)) return HGS_EINVAL;
  if (a.B == 0) return HGS_OK;
  if (!a.rast_in || !a.image || ((uintptr_t)a.rast_in & 15) || (a.F > 0 && !a.faces)) return HGS_EINVAL;
  if (a.C < 1 || a.C > HGS_MESHVIEW_MAX_ATTR || (a.attr_stride != 0 && a.attr_stride != (long long)a.V * a.C)) return HGS_EINVAL;
  if (a.F > 0 && a.V > 0 && !a.attr) return HGS_EINVAL;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const long long n = (long long)a.B * a.H * a.W;
  hipLaunchKernelGGL(hgs_k_mv_interpolate, dim3((unsigned)((n + HGS_MV_THREADS - 1) / HGS_MV_THREADS)), dim3(HGS_MV_THREADS), 0,
                     stream, a);
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}


namespace {
// one scratch buffer for every hgs_meshclean_* call of a mesh
struct MclCarve {
  size_t cbox, vert_keep, face_keep, vert_src, face_src, new_of_old, bsum_v, bsum_f, cell_of, rep, sums, cnt, table_v,
      table_f, total;
  uint32_t cap_v, cap_f;
};
// capacity of a hash table of n items: the power of two in [2 n, 4 n), at least 64
uint32_t mcl_capacity(size_t n) {
  uint32_t c = 64;
  while ((size_t)c < 2 * n) c <<= 1;
  return c;
}
bool mcl_sizes_ok(int32_t V, int32_t F) { return V >= 0 && F >= 0 && V <= HGS_MESHCLEAN_MAX_ITEMS && F <= HGS_MESHCLEAN_MAX_ITEMS; }
MclCarve carve_mcl(int32_t V, int32_t F) {
  MclCarve c;
  const size_t v = (size_t)V, f = (size_t)F;
  c.cap_v = mcl_capacity(v);
  c.cap_f = mcl_capacity(f);
  Carver cv;
  c.cbox = cv.take(v * 32);
  c.vert_keep = cv.take(v);
  c.face_keep = cv.take(f);
  c.vert_src = cv.take(v * 4);
  c.face_src = cv.take(f * 4);
  c.new_of_old = cv.take(v * 4);
  c.bsum_v = cv.take(scan_shape(v, 4).bsum_bytes);
  c.bsum_f = cv.take(scan_shape(f, 4).bsum_bytes);
  c.cell_of = cv.take(v * 4);
  c.rep = cv.take(v * 4);
  c.sums = cv.take(v * 24);
  c.cnt = cv.take(v * 4);
  c.table_v = cv.take((size_t)c.cap_v * 4);
  c.table_f = cv.take((size_t)c.cap_f * 4);
  c.total = cv.off;
  return c;
}
extern "C++" {
template <class T> T* mcl_at(void* scratch, size_t off) { return reinterpret_cast<T*>(static_cast<char*>(scratch) + off); }
}
unsigned mcl_blocks(int32_t n) { return (unsigned)((n + 255) / 256); }
bool mcl_args_ok(const hgs_meshclean_args* a) {
  return a && mcl_sizes_ok(a->V, a->F) && a->info && (a->V == 0 || a->vertices) && (a->F == 0 || a->faces);
}
// keep[n] -> src[0 .. *num) = the kept indices in ascending order (hgs_compact_index's three launches)
void mcl_compact(int32_t n, const uint8_t* keep, int32_t* src, uint32_t* num, uint32_t* bsum, hipStream_t stream) {
  const int nb = (int)scan_shape((size_t)n, 4).blocks;
  hipLaunchKernelGGL(hgs_k_keep_count, dim3(nb), dim3(1024), 0, stream, (int)n, keep, bsum);
  hipLaunchKernelGGL(hgs_k_keep_scan, dim3(1), dim3(1024), 0, stream, nb, bsum, num);
  hipLaunchKernelGGL(hgs_k_keep_index, dim3(nb), dim3(1024), 0, stream, (int)n, keep, bsum, src);
}
bool mcl_info_ok(const hgs_meshclean_args& a, const hgs_meshclean_info* in) {
  return in && in->error == 0 && in->bad_faces == 0 && in->num_vertices <= (uint32_t)a.V && in->num_faces <= (uint32_t)a.F;
}
}  // namespace

size_t hgs_meshclean_scratch_bytes(int32_t V, int32_t F) { return mcl_sizes_ok(V, F) ? carve_mcl(V, F).total : 0; }

int hgs_meshclean_begin(const hgs_meshclean_args* args, void* stream_) {
  if (!mcl_args_ok(args)) return HGS_EINVAL;
  const hgs_meshclean_args& a = *args;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const hipError_t e = box_init(a.info, sizeof(hgs_meshclean_info), a.info->bmin, stream);
  if (e != hipSuccess) return hip_rc(e);
  if (a.V > 0) hipLaunchKernelGGL(hgs_k_mcl_init, dim3(mcl_blocks(a.V)), dim3(256), 0, stream, (int)a.V, a.vertices, a.labels, a.info);
  if (a.F > 0) hipLaunchKernelGGL(hgs_k_mcl_bad_faces, dim3(mcl_blocks(a.F)), dim3(256), 0, stream, (int)a.V, (int)a.F, a.faces, a.info);
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

int hgs_meshclean_rounds(const hgs_meshclean_args* args, int32_t rounds, uint32_t* changed, void* stream_) {
  if (!mcl_args_ok(args) || rounds < 1 || rounds > 64 || !changed) return HGS_EINVAL;
  const hgs_meshclean_args& a = *args;
  if (a.V > 0 && !a.labels) return HGS_EINVAL;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const hipError_t e = hipMemsetAsync(changed, 0, (size_t)rounds * 4, stream);
  if (e != hipSuccess) return hip_rc(e);
  if (a.V == 0 || a.F == 0) return HGS_OK;
  for (int r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(hgs_k_mcl_hook, dim3(mcl_blocks(a.F)), dim3(256), 0, stream, (int)a.V, (int)a.F, a.faces, a.labels, changed + r);
    hipLaunchKernelGGL(hgs_k_mcl_jump, dim3(mcl_blocks(a.V)), dim3(256), 0, stream, (int)a.V, a.labels, changed + r);
  }
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

int hgs_meshclean_components(const hgs_meshclean_args* args, void* stream_) {
  if (!mcl_args_ok(args)) return HGS_EINVAL;
  const hgs_meshclean_args& a = *args;
  if (a.V == 0) return HGS_OK;
  if (!a.labels || !a.comp_faces || !a.comp_diag2 || !a.scratch) return HGS_EINVAL;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const MclCarve c = carve_mcl(a.V, a.F);
  uint32_t* cbox = mcl_at<uint32_t>(a.scratch, c.cbox);
  hipLaunchKernelGGL(hgs_k_mcl_comp_clear, dim3(mcl_blocks(a.V)), dim3(256), 0, stream, (int)a.V, cbox, a.comp_faces);
  hipLaunchKernelGGL(hgs_k_mcl_comp_box, dim3(mcl_blocks(a.V)), dim3(256), 0, stream, (int)a.V, a.vertices, a.labels, cbox);
  if (a.F > 0)
    hipLaunchKernelGGL(hgs_k_mcl_comp_faces, dim3(mcl_blocks(a.F)), dim3(256), 0, stream, (int)a.V, (int)a.F, a.faces, a.labels, a.comp_faces);
  hipLaunchKernelGGL(hgs_k_mcl_comp_diag, dim3(mcl_blocks(a.V)), dim3(256), 0, stream, (int)a.V, a.labels, cbox, a.comp_diag2);
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

int hgs_meshclean_clean_mark(const hgs_meshclean_args* args, void* stream_) {
  if (!mcl_args_ok(args)) return HGS_EINVAL;
  const hgs_meshclean_args& a = *args;
  if (a.V == 0 || a.F == 0) return HGS_OK;                 // (info->num_* are 0 since hgs_meshclean_begin)
  if (!a.labels || !a.comp_faces || !a.comp_diag2 || !a.scratch) return HGS_EINVAL;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const MclCarve c = carve_mcl(a.V, a.F);
  uint8_t* vert_keep = mcl_at<uint8_t>(a.scratch, c.vert_keep);
  uint8_t* face_keep = mcl_at<uint8_t>(a.scratch, c.face_keep);
  const hipError_t e = hipMemsetAsync(vert_keep, 0, (size_t)a.V, stream);
  if (e != hipSuccess) return hip_rc(e);
  hipLaunchKernelGGL(hgs_k_mcl_clean_mark, dim3(mcl_blocks(a.F)), dim3(256), 0, stream, (int)a.V, (int)a.F, a.faces, a.labels,
                     a.comp_faces, a.comp_diag2, a.info, (int)a.min_f, a.min_d, face_keep, vert_keep);
  mcl_compact(a.V, vert_keep, mcl_at<int32_t>(a.scratch, c.vert_src), &a.info->num_vertices, mcl_at<uint32_t>(a.scratch, c.bsum_v), stream);
  mcl_compact(a.F, face_keep, mcl_at<int32_t>(a.scratch, c.face_src), &a.info->num_faces, mcl_at<uint32_t>(a.scratch, c.bsum_f), stream);
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

int hgs_meshclean_clean_emit(const hgs_meshclean_args* args, const hgs_meshclean_info* info_host, void* stream_) {
  if (!mcl_args_ok(args) || !mcl_info_ok(*args, info_host)) return HGS_EINVAL;
  const hgs_meshclean_args& a = *args;
  const int32_t Vn = (int32_t)info_host->num_vertices, Fn = (int32_t)info_host->num_faces;
  if (Vn == 0 && Fn == 0) return HGS_OK;
  if (!a.scratch || (Vn > 0 && !a.vertices_out) || (Fn > 0 && (!a.faces_out || Vn == 0))) return HGS_EINVAL;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const MclCarve c = carve_mcl(a.V, a.F);
  const int32_t* vert_src = mcl_at<int32_t>(a.scratch, c.vert_src);
  int32_t* new_of_old = mcl_at<int32_t>(a.scratch, c.new_of_old);
  const long long nf = 3ll * Vn;
  hipLaunchKernelGGL(hgs_k_gather_rows, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, stream, nf, 3, vert_src, a.vertices,
                     a.vertices_out);
  hipLaunchKernelGGL(hgs_k_mcl_invert, dim3(mcl_blocks(Vn)), dim3(256), 0, stream, (int)Vn, vert_src, new_of_old, a.vertex_src);
  if (Fn > 0)
    hipLaunchKernelGGL(hgs_k_mcl_faces_out, dim3((unsigned)((3ll * Fn + 255) / 256)), dim3(256), 0, stream, (int)Fn,
                       mcl_at<const int32_t>(a.scratch, c.face_src), a.faces, static_cast<const int32_t*>(nullptr), new_of_old,
                       a.faces_out);
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

int hgs_meshclean_count(const hgs_meshclean_args* args, const int32_t* g, uint32_t* counts, void* stream_) {
  if (!mcl_args_ok(args) || !g || !counts) return HGS_EINVAL;
  const hgs_meshclean_args& a = *args;
  MclProbe probe;
  bool any = false;
  for (int k = 0; k < 3; ++k) {
    if (g[k] > HGS_MESHCLEAN_G_MAX) return HGS_EINVAL;
    probe.g[k] = g[k] < 1 ? 0 : g[k];
    any = any || probe.g[k] > 0;
  }
  if (a.V == 0 || a.F == 0 || !any) return HGS_OK;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(hgs_k_mcl_count, dim3(mcl_blocks(a.F)), dim3(256), 0, stream, (int)a.V, a.vertices, (int)a.F, a.faces,
                     a.info, probe, counts);
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

int hgs_meshclean_decimate_mark(const hgs_meshclean_args* args, int32_t g, void* stream_) {
  if (!mcl_args_ok(args) || g < 1 || g > HGS_MESHCLEAN_G_MAX) return HGS_EINVAL;
  const hgs_meshclean_args& a = *args;
  if (a.V == 0 || a.F == 0) return HGS_OK;
  if (!a.scratch) return HGS_EINVAL;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const MclCarve c = carve_mcl(a.V, a.F);
  uint32_t* table_v = mcl_at<uint32_t>(a.scratch, c.table_v);
  uint32_t* table_f = mcl_at<uint32_t>(a.scratch, c.table_f);
  uint32_t* cell_of = mcl_at<uint32_t>(a.scratch, c.cell_of);
  int32_t* rep = mcl_at<int32_t>(a.scratch, c.rep);
  unsigned long long* sums = mcl_at<unsigned long long>(a.scratch, c.sums);
  uint32_t* cnt = mcl_at<uint32_t>(a.scratch, c.cnt);
  uint8_t* rep_used = mcl_at<uint8_t>(a.scratch, c.vert_keep);
  uint8_t* face_keep = mcl_at<uint8_t>(a.scratch, c.face_keep);
  hipError_t e = hipMemsetAsync(table_v, 0xff, (size_t)c.cap_v * 4, stream);
  if (e == hipSuccess) e = hipMemsetAsync(table_f, 0xff, (size_t)c.cap_f * 4, stream);
  if (e == hipSuccess) e = hipMemsetAsync(sums, 0, (size_t)a.V * 24, stream);
  if (e == hipSuccess) e = hipMemsetAsync(cnt, 0, (size_t)a.V * 4, stream);
  if (e == hipSuccess) e = hipMemsetAsync(rep_used, 0, (size_t)a.V, stream);
  if (e != hipSuccess) return hip_rc(e);
  const unsigned gv = mcl_blocks(a.V), gf = mcl_blocks(a.F);
  hipLaunchKernelGGL(hgs_k_mcl_cell_insert, dim3(gv), dim3(256), 0, stream, (int)a.V, a.vertices, a.info, (int)g, c.cap_v, table_v, cell_of);
  hipLaunchKernelGGL(hgs_k_mcl_cell_lookup, dim3(gv), dim3(256), 0, stream, (int)a.V, a.vertices, a.info, c.cap_v, table_v, cell_of, rep, sums, cnt);
  hipLaunchKernelGGL(hgs_k_mcl_face_insert, dim3(gf), dim3(256), 0, stream, (int)a.V, (int)a.F, a.faces, rep, a.info, c.cap_f, table_f);
  hipLaunchKernelGGL(hgs_k_mcl_face_mark, dim3(gf), dim3(256), 0, stream, (int)a.V, (int)a.F, a.faces, rep, a.info, c.cap_f, table_f, face_keep, rep_used);
  mcl_compact(a.V, rep_used, mcl_at<int32_t>(a.scratch, c.vert_src), &a.info->num_vertices, mcl_at<uint32_t>(a.scratch, c.bsum_v), stream);
  mcl_compact(a.F, face_keep, mcl_at<int32_t>(a.scratch, c.face_src), &a.info->num_faces, mcl_at<uint32_t>(a.scratch, c.bsum_f), stream);
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

int hgs_meshclean_decimate_emit(const hgs_meshclean_args* args, const hgs_meshclean_info* info_host, void* stream_) {
  if (!mcl_args_ok(args) || !mcl_info_ok(*args, info_host)) return HGS_EINVAL;
  const hgs_meshclean_args& a = *args;
  const int32_t Vn = (int32_t)info_host->num_vertices, Fn = (int32_t)info_host->num_faces;
  if (Vn == 0 && Fn == 0) return HGS_OK;
  if (!a.scratch || (Vn > 0 && !a.vertices_out) || (Fn > 0 && (!a.faces_out || Vn == 0))) return HGS_EINVAL;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const MclCarve c = carve_mcl(a.V, a.F);
  int32_t* new_of_old = mcl_at<int32_t>(a.scratch, c.new_of_old);
  hipLaunchKernelGGL(hgs_k_mcl_cell_means, dim3(mcl_blocks(Vn)), dim3(256), 0, stream, (int)Vn,
                     mcl_at<const int32_t>(a.scratch, c.vert_src), a.info, mcl_at<const unsigned long long>(a.scratch, c.sums),
                     mcl_at<const uint32_t>(a.scratch, c.cnt), new_of_old, a.vertices_out);
  if (Fn > 0)
    hipLaunchKernelGGL(hgs_k_mcl_faces_out, dim3((unsigned)((3ll * Fn + 255) / 256)), dim3(256), 0, stream, (int)Fn,
                       mcl_at<const int32_t>(a.scratch, c.face_src), a.faces, mcl_at<const int32_t>(a.scratch, c.rep), new_of_old,
                       a.faces_out);
  HGS_LAUNCH_CHECK();
  return HGS_OK;
}

}  // extern "C"
