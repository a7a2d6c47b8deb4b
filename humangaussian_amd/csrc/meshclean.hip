// meshclean.hip - what follows marching cubes in the reference's extract_mesh (gs_renderer.py:333-361: kiui's clean_mesh
// and decimate_mesh, pymeshlab on the CPU): the floaters of the iso-surface removed by connected components, the mesh
// decimated to a face budget by vertex clustering on a uniform grid.  include/hgs_rast.h (hgs_meshclean_*) states the
// semantics operation by operation; tests/mesh_clean_reference.py restates them in numpy.
//
// Rules every kernel here keeps (a union / hash kernel is the classic way to hang a card):
//   - no thread waits for another: no spin loops, no locks.  Every loop has a trip bound written in the code (a hash
//     probe: the table's capacity); running into it sets a bit of hgs_meshclean_info::error and the thread moves on.
//   - components are ROUNDS OF LAUNCHES (hook the faces' labels and their roots with atomicMin, then one pointer-jumping
//     pass); labels only decrease, a stale read inside a round can only delay a decrease, and the round that changes
//     nothing has read settled values only.  The host reads the rounds' change counters.
//   - a hash table is built from the RETURNED values of its atomics only (atomicCAS, then atomicMin into a slot of the
//     item's own class); it is looked up in a later launch.
//   - sums that decide output bits are integer atomics (ordered float keys for the boxes, 64-bit lattice sums for the
//     means): no float atomics, nothing depends on arrival order.
#include "hgs_common.h"
#include "gridscan.h"

#define HGS_MCL_EMPTY 0xffffffffu

// the box of an info block (or of a component) as floats
struct MclBox { float lo[3], ext[3], emax; };
__device__ __forceinline__ MclBox hgs_mcl_box(const uint32_t* bmin, const uint32_t* bmax) {
  MclBox b;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    b.lo[a] = hgs_key_float(bmin[a]);
    b.ext[a] = hgs_key_float(bmax[a]) - b.lo[a];
  }
  b.emax = fmaxf(b.ext[0], fmaxf(b.ext[1], b.ext[2]));
  return b;
}
// squared diagonal of a box of keys: (dx dx + dy dy) + dz dz, fp32 (0 + dx dx is dx dx); an empty box (no finite vertex): 0.
// (The axes stay a loop: unrolled, the vectorised key decoding takes down this compiler's instruction selection.)
__device__ __forceinline__ float hgs_mcl_diag2(const uint32_t* bmin, const uint32_t* bmax) {
  if (bmin[0] > bmax[0]) return 0.0f;
  float d2 = 0.0f;
#pragma unroll 1
  for (int a = 0; a < 3; ++a) {
    const float d = hgs_key_float(bmax[a]) - hgs_key_float(bmin[a]);
    d2 = d2 + d * d;
  }
  return d2;
}
__device__ __forceinline__ bool hgs_mcl_finite3(float x, float y, float z) {
  return fabsf(x) <= 3.402823466e38f && fabsf(y) <= 3.402823466e38f && fabsf(z) <= 3.402823466e38f;
}
__device__ __forceinline__ bool hgs_mcl_face(const int32_t* __restrict__ faces, int f, int V, int& a, int& b, int& c) {
  a = faces[3 * f]; b = faces[3 * f + 1]; c = faces[3 * f + 2];
  return a >= 0 && a < V && b >= 0 && b < V && c >= 0 && c < V;
}
// a label another thread of the launch may lower: read past this CU's L1 (a stale value would only delay the round)
__device__ __forceinline__ int hgs_mcl_label(const int32_t* labels, int v) {
  return __hip_atomic_load(labels + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void hgs_mcl_flag(bool changed, uint32_t* counter) {
  if (__ballot(changed) != 0ull && (threadIdx.x & 63) == 0) atomicAdd(counter, 1u);
}
__device__ __forceinline__ uint32_t hgs_mcl_mix(uint32_t h) {
  h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
  return h;
}

// ---- components ------------------------------------------------------------------------------------------------------
// labels[v] = v; the box of the finite vertices into info (hgs_box_reduce: every lane of the wave calls it)
extern "C" __global__ void __launch_bounds__(256)
hgs_k_mcl_init(int V, const float* __restrict__ vertices, int32_t* __restrict__ labels, hgs_meshclean_info* info) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  float x = 0.0f, y = 0.0f, z = 0.0f;
  if (v < V) {
    x = vertices[3 * v]; y = vertices[3 * v + 1]; z = vertices[3 * v + 2];
    if (labels) labels[v] = v;
  }
  hgs_box_reduce(v < V && hgs_mcl_finite3(x, y, z), x, y, z, info->bmin, info->bmax);
}

extern "C" __global__ void __launch_bounds__(256)
hgs_k_mcl_bad_faces(int V, int F, const int32_t* __restrict__ faces, hgs_meshclean_info* info) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  int a, b, c;
  const bool bad = f < F && !hgs_mcl_face(faces, f, V, a, b, c);
  const unsigned long long m = __ballot(bad);
  if (m != 0ull && (threadIdx.x & 63) == 0) atomicAdd(&info->bad_faces, (uint32_t)__popcll(m));
}

// one round, first half: m = the smallest of the face's three labels goes into the three labels and into the labels'
// own labels (the roots are hooked).  A label that already equals m is at most m for good and is left alone.
extern "C" __global__ void __launch_bounds__(256)
hgs_k_mcl_hook(int V, int F, const int32_t* __restrict__ faces, int32_t* labels, uint32_t* changed) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  bool ch = false;
  int idx[3];
  if (f < F && hgs_mcl_face(faces, f, V, idx[0], idx[1], idx[2])) {
    int l[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) l[k] = hgs_mcl_label(labels, idx[k]);
    const int m = min(l[0], min(l[1], l[2]));
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (l[k] > m) {
        ch |= atomicMin(&labels[idx[k]], m) > m;
        // (the root of a large patch is hooked by every face on the patch's rim: look first - a load is served beside the
        //  others, the atomics on one word queue up; a stale look only costs the atomic it would have saved)
        if (hgs_mcl_label(labels, l[k]) > m) ch |= atomicMin(&labels[l[k]], m) > m;
      }
    }
  }
  hgs_mcl_flag(ch, changed);
}

// one round, second half: ONE pointer-jumping pass, labels[v] = labels[labels[v]]
extern "C" __global__ void __launch_bounds__(256)
hgs_k_mcl_jump(int V, int32_t* labels, uint32_t* changed) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  bool ch = false;
  if (v < V) {
    const int l = hgs_mcl_label(labels, v);
    const int ll = hgs_mcl_label(labels, l);
    if (ll < l) ch = atomicMin(&labels[v], ll) > ll;
  }
  hgs_mcl_flag(ch, changed);
}

// per component, at its label: the box of its finite vertices (n = V threads) ...  A wave whose vertices all carry ONE
// label - the rule on a mesh with few components - reduces on chip and issues one atomic per axis and bound
// (hgs_box_reduce); thousands of lanes on the six words of one component would queue up behind each other.  A mixed
// wave issues its lanes' atomics.  Integer min / max either way: the same bits.
extern "C" __global__ void __launch_bounds__(256)
hgs_k_mcl_comp_box(int V, const float* __restrict__ vertices, const int32_t* __restrict__ labels, uint32_t* cbox) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  float x = 0.0f, y = 0.0f, z = 0.0f;
  int L = -1;
  if (v < V) { x = vertices[3 * v]; y = vertices[3 * v + 1]; z = vertices[3 * v + 2]; L = labels[v]; }
  const bool take = v < V && hgs_mcl_finite3(x, y, z);
  const unsigned long long takers = __ballot(take);
  if (takers == 0ull) return;                                  // (wave-uniform)
  const int L0 = __shfl(L, __ffsll((long long)takers) - 1);
  if (__ballot(take && L != L0) == 0ull) {                      // (wave-uniform)
    hgs_box_reduce(take, x, y, z, cbox + 8 * (size_t)L0, cbox + 8 * (size_t)L0 + 4);
  } else if (take) {
    uint32_t* box = cbox + 8 * (size_t)L;
    const uint32_t k[3] = {hgs_float_key(x), hgs_float_key(y), hgs_float_key(z)};
#pragma unroll
    for (int a = 0; a < 3; ++a) { atomicMin(&box[a], k[a]); atomicMax(&box[4 + a], k[a]); }
  }
}
// ... and the number of its faces (n = F threads), one add per wave where the wave's faces share a label
extern "C" __global__ void __launch_bounds__(256)
hgs_k_mcl_comp_faces(int V, int F, const int32_t* __restrict__ faces, const int32_t* __restrict__ labels,
                     int32_t* comp_faces) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  int a, b, c;
  const bool take = f < F && hgs_mcl_face(faces, f, V, a, b, c);
  const int L = take ? labels[a] : -1;
  const unsigned long long takers = __ballot(take);
  if (takers == 0ull) return;                                  // (wave-uniform)
  const int L0 = __shfl(L, __ffsll((long long)takers) - 1);
  if (__ballot(take && L != L0) == 0ull) {
    if ((threadIdx.x & 63) == 0) atomicAdd(&comp_faces[L0], (int)__popcll(takers));
  } else if (take) {
    atomicAdd(&comp_faces[L], 1);
  }
}
// cbox rows (32 bytes: bmin, pad, bmax, pad): empty boxes (bmin all ones, bmax 0); comp_faces: 0
extern "C" __global__ void __launch_bounds__(256)
hgs_k_mcl_comp_clear(int V, uint32_t* cbox, int32_t* comp_faces) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= V) return;
#pragma unroll
  for (int a = 0; a < 4; ++a) { cbox[8 * (size_t)v + a] = 0xffffffffu; cbox[8 * (size_t)v + 4 + a] = 0u; }
  comp_faces[v] = 0;
}
extern "C" __global__ void __launch_bounds__(256)
hgs_k_mcl_comp_diag(int V, const int32_t* __restrict__ labels, const uint32_t* __restrict__ cbox, float* comp_diag2) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= V) return;
  const float d2 = labels[v] == v ? hgs_mcl_diag2(cbox + 8 * (size_t)v, cbox + 8 * (size_t)v + 4) : 0.0f;
  comp_diag2[v] = d2;
}

// ---- clean: the keep rule ----------------------------------------------------------------------------------------------
// vert_keep is zero on entry; every thread that sets a byte writes the same 1
extern "C" __global__ void __launch_bounds__(256)
hgs_k_mcl_clean_mark(int V, int F, const int32_t* __restrict__ faces, const int32_t* __restrict__ labels,
                     const int32_t* __restrict__ comp_faces, const float* __restrict__ comp_diag2,
                     const hgs_meshclean_info* __restrict__ info, int min_f, float min_d, uint8_t* face_keep,
                     uint8_t* vert_keep) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  int a, b, c;
  bool keep = hgs_mcl_face(faces, f, V, a, b, c) && a != b && b != c && a != c;
  if (keep) {
    const int L = labels[a];
    const float p = min_d / 100.0f;
    const float thr = (p * p) * hgs_mcl_diag2(info->bmin, info->bmax);
    keep = comp_faces[L] >= min_f && !(comp_diag2[L] < thr);
  }
  face_keep[f] = keep ? 1 : 0;
  if (keep) { vert_keep[a] = 1; vert_keep[b] = 1; vert_keep[c] = 1; }
}

// ---- what clean and decimate share: the output's indices ------------------------------------------------------------------
// new_of_old[vertex_src[j]] = j; vertex_src_out (optional) = a copy for the caller
extern "C" __global__ void __launch_bounds__(256)
hgs_k_mcl_invert(int n, const int32_t* __restrict__ vertex_src, int32_t* __restrict__ new_of_old,
                 int32_t* __restrict__ vertex_src_out) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const int s = vertex_src[j];
  new_of_old[s] = j;
  if (vertex_src_out) vertex_src_out[j] = s;
}
// faces_out[i] = the kept face face_src[i], its indices taken through rep (decimate; NULL: clean) and new_of_old
extern "C" __global__ void __launch_bounds__(256)
hgs_k_mcl_faces_out(int n, const int32_t* __restrict__ face_src, const int32_t* __restrict__ faces,
                    const int32_t* __restrict__ rep, const int32_t* __restrict__ new_of_old, int32_t* __restrict__ faces_out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= 3 * n) return;
  const int i = e / 3, k = e - 3 * i;
  int v = faces[3 * face_src[i] + k];
  if (rep) v = rep[v];
  faces_out[e] = new_of_old[v];
}

// ---- decimate: vertex clustering ----------------------------------------------------------------------------------------
// the grid of g cells per axis over the box: cells of edge emax / g from the box minimum
struct MclGrid { float lo[3], inv_h; int g; };
__device__ __forceinline__ MclGrid hgs_mcl_grid(const hgs_meshclean_info* info, int g) {
  const MclBox b = hgs_mcl_box(info->bmin, info->bmax);
  MclGrid G;
  G.lo[0] = b.lo[0]; G.lo[1] = b.lo[1]; G.lo[2] = b.lo[2];
  G.inv_h = (float)g / b.emax;
  G.g = g;
  return G;
}
// 30-bit cell key of vertex v: (cz g + cy) g + cx
__device__ __forceinline__ uint32_t hgs_mcl_cell(const MclGrid& G, const float* __restrict__ vertices, int v) {
  const int cx = hgs_grid_cell1(vertices[3 * v], G.lo[0], G.inv_h, G.g);
  const int cy = hgs_grid_cell1(vertices[3 * v + 1], G.lo[1], G.inv_h, G.g);
  const int cz = hgs_grid_cell1(vertices[3 * v + 2], G.lo[2], G.inv_h, G.g);
  return ((uint32_t)cz * (uint32_t)G.g + (uint32_t)cy) * (uint32_t)G.g + (uint32_t)cx;
}

// counts[k] += faces whose three vertices lie in three different cells of grid g[k], k < 3 (g[k] < 1: not asked)
struct MclProbe { int g[3]; };
extern "C" __global__ void __launch_bounds__(256)
hgs_k_mcl_count(int V, const float* __restrict__ vertices, int F, const int32_t* __restrict__ faces,
                const hgs_meshclean_info* __restrict__ info, MclProbe probe, uint32_t* counts) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  int a, b, c;
  const bool valid = f < F && hgs_mcl_face(faces, f, V, a, b, c);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (probe.g[k] < 1) continue;                    // (uniform)
    bool s = false;
    if (valid) {
      const MclGrid G = hgs_mcl_grid(info, probe.g[k]);
      const uint32_t ka = hgs_mcl_cell(G, vertices, a), kb = hgs_mcl_cell(G, vertices, b), kc = hgs_mcl_cell(G, vertices, c);
      s = ka != kb && kb != kc && ka != kc;
    }
    const unsigned long long m = __ballot(s);
    if (m != 0ull && (threadIdx.x & 63) == 0) atomicAdd(&counts[k], (uint32_t)__popcll(m));
  }
}

// Table of the cells: a slot holds the lowest vertex of its cell.  Insertion of vertex v, at most `cap` probes.
extern "C" __global__ void __launch_bounds__(256)
hgs_k_mcl_cell_insert(int V, const float* __restrict__ vertices, hgs_meshclean_info* info, int g, uint32_t cap,
                      uint32_t* table, uint32_t* __restrict__ cell_of) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= V) return;
  const MclGrid G = hgs_mcl_grid(info, g);
  const uint32_t key = hgs_mcl_cell(G, vertices, v);
  cell_of[v] = key;
  uint32_t slot = hgs_mcl_mix(key) & (cap - 1);
  bool done = false;
  for (uint32_t probe = 0; probe < cap && !done; ++probe) {
    const uint32_t cur = atomicCAS(&table[slot], HGS_MCL_EMPTY, (uint32_t)v);
    if (cur == HGS_MCL_EMPTY) {
      done = true;
    } else if (cur < (uint32_t)V && hgs_mcl_cell(G, vertices, (int)cur) == key) {   // (the class from the immutable input)
      atomicMin(&table[slot], (uint32_t)v);
      done = true;
    } else {
      slot = (slot + 1) & (cap - 1);
    }
  }
  if (!done) atomicOr(&info->error, HGS_MESHCLEAN_ERR_CELL_TABLE);
}

// A later launch: rep[v] = the lowest vertex of v's cell; the cell's lattice sums and its count, at rep[v].
// Lattice: q = clamp(floorf((x - lo) * (1048576 / emax) + 0.5), 0, 1048576) per axis, fp32; NaN -> 0.
extern "C" __global__ void __launch_bounds__(256)
hgs_k_mcl_cell_lookup(int V, const float* __restrict__ vertices, hgs_meshclean_info* info, uint32_t cap,
                      const uint32_t* __restrict__ table, const uint32_t* __restrict__ cell_of, int32_t* __restrict__ rep,
                      unsigned long long* sums, uint32_t* cnt) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= V) return;
  const uint32_t key = cell_of[v];
  uint32_t slot = hgs_mcl_mix(key) & (cap - 1);
  int r = -1;
  for (uint32_t probe = 0; probe < cap && r < 0; ++probe) {
    const uint32_t cur = table[slot];
    if (cur == HGS_MCL_EMPTY || cur >= (uint32_t)V) break;
    if (cell_of[cur] == key) r = (int)cur;
    slot = (slot + 1) & (cap - 1);
  }
  if (r < 0) { atomicOr(&info->error, HGS_MESHCLEAN_ERR_CELL_TABLE); r = v; }
  rep[v] = r;
  const MclBox b = hgs_mcl_box(info->bmin, info->bmax);
  const float qs = 1048576.0f / b.emax;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float q = fminf(fmaxf(floorf((vertices[3 * v + a] - b.lo[a]) * qs + 0.5f), 0.0f), 1048576.0f);
    atomicAdd(&sums[3 * (size_t)r + a], (unsigned long long)q);
  }
  atomicAdd(&cnt[r], 1u);
}

// the class of a face: its three representatives in ascending order; false: not a surviving face
__device__ __forceinline__ bool hgs_mcl_face_class(const int32_t* __restrict__ faces, const int32_t* __restrict__ rep, int f,
                                                   int V, uint32_t& lo, uint32_t& mid, uint32_t& hi) {
  int a, b, c;
  if (!hgs_mcl_face(faces, f, V, a, b, c)) return false;
  const uint32_t ra = (uint32_t)rep[a], rb = (uint32_t)rep[b], rc = (uint32_t)rep[c];
  if (ra == rb || rb == rc || ra == rc) return false;
  lo = min(ra, min(rb, rc));
  hi = max(ra, max(rb, rc));
  mid = ra ^ rb ^ rc ^ lo ^ hi;
  return true;
}
__device__ __forceinline__ uint32_t hgs_mcl_face_hash(uint32_t lo, uint32_t mid, uint32_t hi) {
  return hgs_mcl_mix(hgs_mcl_mix(hgs_mcl_mix(lo) ^ (mid * 0x9e3779b1u)) ^ (hi * 0x85ebca77u));
}

// Table of the vertex sets: a slot holds the lowest surviving face of its set.  At most `cap` probes.
extern "C" __global__ void __launch_bounds__(256)
hgs_k_mcl_face_insert(int V, int F, const int32_t* __restrict__ faces, const int32_t* __restrict__ rep,
                      hgs_meshclean_info* info, uint32_t cap, uint32_t* table) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  uint32_t lo, mid, hi;
  if (f >= F || !hgs_mcl_face_class(faces, rep, f, V, lo, mid, hi)) return;
  uint32_t slot = hgs_mcl_face_hash(lo, mid, hi) & (cap - 1);
  bool done = false;
  for (uint32_t probe = 0; probe < cap && !done; ++probe) {
    const uint32_t cur = atomicCAS(&table[slot], HGS_MCL_EMPTY, (uint32_t)f);
    uint32_t l2, m2, h2;
    if (cur == HGS_MCL_EMPTY) {
      done = true;
    } else if (cur < (uint32_t)F && hgs_mcl_face_class(faces, rep, (int)cur, V, l2, m2, h2) && l2 == lo && m2 == mid && h2 == hi) {
      atomicMin(&table[slot], (uint32_t)f);
      done = true;
    } else {
      slot = (slot + 1) & (cap - 1);
    }
  }
  if (!done) atomicOr(&info->error, HGS_MESHCLEAN_ERR_FACE_TABLE);
}

// A later launch: a surviving face stays iff it is the lowest of its vertex set; its three cells get a new vertex.
// face_keep is written for every face; rep_used is zero on entry.
extern "C" __global__ void __launch_bounds__(256)
hgs_k_mcl_face_mark(int V, int F, const int32_t* __restrict__ faces, const int32_t* __restrict__ rep,
                    hgs_meshclean_info* info, uint32_t cap, const uint32_t* __restrict__ table, uint8_t* face_keep,
                    uint8_t* rep_used) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  uint32_t lo, mid, hi;
  bool keep = false;
  if (hgs_mcl_face_class(faces, rep, f, V, lo, mid, hi)) {
    uint32_t slot = hgs_mcl_face_hash(lo, mid, hi) & (cap - 1);
    bool found = false;
    for (uint32_t probe = 0; probe < cap && !found; ++probe) {
      const uint32_t cur = table[slot];
      uint32_t l2, m2, h2;
      if (cur == HGS_MCL_EMPTY || cur >= (uint32_t)F) break;
      if (hgs_mcl_face_class(faces, rep, (int)cur, V, l2, m2, h2) && l2 == lo && m2 == mid && h2 == hi) {
        found = true;
        keep = cur == (uint32_t)f;
      }
      slot = (slot + 1) & (cap - 1);
    }
    if (!found) atomicOr(&info->error, HGS_MESHCLEAN_ERR_FACE_TABLE);
  }
  face_keep[f] = keep ? 1 : 0;
  if (keep) { rep_used[lo] = 1; rep_used[mid] = 1; rep_used[hi] = 1; }
}

// new vertex j = the mean of the cell of representative vertex_src[j]: m = (double)sum / (double)count per axis,
// position = (float)((double)lo + m * ((double)emax / 1048576.0)); new_of_old[vertex_src[j]] = j
extern "C" __global__ void __launch_bounds__(256)
hgs_k_mcl_cell_means(int n, const int32_t* __restrict__ vertex_src, const hgs_meshclean_info* __restrict__ info,
                     const unsigned long long* __restrict__ sums, const uint32_t* __restrict__ cnt,
                     int32_t* __restrict__ new_of_old, float* __restrict__ vertices_out) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const int r = vertex_src[j];
  new_of_old[r] = j;
  const MclBox b = hgs_mcl_box(info->bmin, info->bmax);
  const double step = (double)b.emax / 1048576.0;
  const double c = (double)cnt[r];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double m = (double)sums[3 * (size_t)r + a] / c;
    vertices_out[3 * j + a] = (float)((double)b.lo[a] + m * step);
  }
}
