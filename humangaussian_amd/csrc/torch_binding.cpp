// torch_binding.cpp - the `_C` module of the reference's extension, re-done on top of the C ABI.
//
// Upstream binds `rasterize_gaussians`, `rasterize_gaussians_backward` and `mark_visible` with
// pybind11 and wraps them in a Python autograd.Function (diff_gaussian_rasterization/__init__.py
// of the ashawkey fork, imported at
// /root/reference/gaussiansplatting/gaussian_renderer/__init__.py:14).  Here the autograd node
// itself lives in C++ (torch::autograd::Function): at 0.3 ms per training-style step the Python
// autograd.Function machinery (apply, ctypes marshalling, GIL hand-off into the engine's device
// thread for backward) cost as much host time as the GPU needs for the whole step.
//
// This file is PLUMBING: it owns tensors, the current HIP stream, the per-device capacity
// estimates and the one host wait per forward.  All arithmetic is behind include/hgs_rast.h
// (libhgs_rast.so); nothing here launches a kernel itself.  Built by g++ (no device code).
#include <torch/extension.h>
#include <c10/hip/HIPFunctions.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <thread>
#include <cstring>
#include <map>
#include <memory>
#include <tuple>
#include <mutex>
#include <utility>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/hgs_rast.h"

namespace {

using torch::Tensor;
using torch::autograd::AutogradContext;
using torch::autograd::variable_list;

constexpr int RING = 64;      // status slots (pinned, 32 B each): a slot stays untouched for the next RING - 1 forwards

// Switch the current HIP device only when it is not already the tensors' device.  (torch's own
// HIPGuard types are keyed on DeviceType::HIP, which the ROCm build masquerades as CUDA.)
struct DeviceSwitch {
  c10::DeviceIndex prev = -1;
  explicit DeviceSwitch(c10::DeviceIndex want) {
    const c10::DeviceIndex cur = c10::hip::current_device();
    if (cur != want) { prev = cur; c10::hip::set_device(want); }
  }
  ~DeviceSwitch() { if (prev >= 0) c10::hip::set_device(prev); }
};

void hip_ok(hipError_t e, const char* what) {
  if (e != hipSuccess)
    throw std::runtime_error(std::string("humangaussian_amd: ") + what + ": " + hipGetErrorString(e));
}

// Workload estimate for one (views, height, width) shape on one device: entry capacity of the bin
// buffer and the longest tile list (sort-class / segment hint).  Both follow the workload with a
// DECAYING maximum, so alternating cameras (wide / head zoom, train / eval resolution) neither
// trip the device-side overflow check every other call nor pin the buffers at a one-off peak.
struct Estimate {
  int64_t capacity = 0;       // entries; 0 = unknown
  int64_t tile_hint = 0;      // 0 = unknown
};

struct DevState {
  std::map<std::tuple<int64_t, int64_t, int64_t>, Estimate> est;   // (B, H, W) -> estimate
  int64_t max_R = 0;          // of the last call
  int64_t max_tile = 0;       // of the last call
  int64_t last_capacity = 0, last_hint = 0;
  Tensor status_ring;         // pinned int32 [RING][8]
  hgs_status* ring = nullptr;
  hipEvent_t status_event = nullptr;          // recorded by the library right behind the tiles stage
  int ring_pos = 0;
  int64_t ring_issued = 0;    // slots handed out so far
  int64_t last_scratch = 0, last_pairs = 0;   // of the last backward (diagnostic)
  int64_t calls = 0;
  int64_t retries = 0;        // forwards that had to be re-run (capacity or hint exceeded)
  int64_t wait_ns = 0;        // host time blocked in the per-forward status wait (diagnostic)
  // host time per phase (diagnostic, bench.py): forward: checks + allocations | hgs_forward (launches) | autograd state
  // in the shadow of the wait | the wait | after it; backward: before | hgs_backward (launches) | after
  std::atomic<int64_t> host_ns[8] = {};
  std::mutex mu;
};

std::mutex g_mu;
std::vector<DevState*> g_states(64, nullptr);
std::vector<void*> g_stage_fwd, g_stage_bwd;

DevState& state_for(int dev) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (dev < 0 || dev >= (int)g_states.size()) throw std::runtime_error("bad device index");
  if (!g_states[dev]) {
    DeviceSwitch guard((c10::DeviceIndex)dev);          // the event belongs to `dev`, whatever device is current
    auto* st = new DevState();
    st->status_ring = at::zeros({RING, 8}, at::TensorOptions().dtype(at::kInt)).pin_memory();
    static_assert(sizeof(hgs_status) == 32, "hgs_status is 8 words");
    st->ring = reinterpret_cast<hgs_status*>(st->status_ring.data_ptr<int32_t>());
    hip_ok(hipEventCreateWithFlags(&st->status_event, hipEventDisableTiming), "hipEventCreate");
    g_states[dev] = st;
  }
  return *g_states[dev];
}

int64_t round_capacity(int64_t n) { return std::max<int64_t>(1 << 16, (n + 0xFFFF) & ~int64_t(0xFFFF)); }
int64_t al256(size_t n) { return (int64_t)((n + 255) & ~size_t(255)); }

Tensor f32c(const Tensor& t, const c10::Device& dev, const char* name) {
  if (t.device() != dev)
    throw std::runtime_error(std::string("expected ") + name + " on " + dev.str() + ", got " + t.device().str());
  Tensor r = t.scalar_type() == at::kFloat ? t : t.to(at::kFloat);
  return r.is_contiguous() ? r : r.contiguous();
}

const float* fptr(const Tensor& t) { return t.defined() && t.numel() > 0 ? t.data_ptr<float>() : nullptr; }
float* fptr_mut(Tensor& t) { return t.defined() && t.numel() > 0 ? t.data_ptr<float>() : nullptr; }

// B camera blocks: settings[b] points into the batched tensors (kept alive here)
struct Settings {
  std::vector<hgs_settings> s;
  Tensor bg, vm, pm, cp;    // (B,3), (B,16), (B,16), (B,3)
};

Settings make_settings(const Tensor& bg, const Tensor& vm, const Tensor& pm, const Tensor& cp, int64_t B, int64_t H,
                       int64_t W, const double* tanfovx, const double* tanfovy, double scale_modifier,
                       int64_t sh_degree, bool prefiltered, bool debug, const c10::Device& dev) {
  if (B < 1 || B > HGS_MAX_VIEWS)
    throw std::runtime_error("a batched call takes 1.." + std::to_string(HGS_MAX_VIEWS) + " views, got " + std::to_string(B));
  Settings r;
  r.vm = f32c(vm, dev, "viewmatrix");
  r.pm = f32c(pm, dev, "projmatrix");
  r.cp = f32c(cp, dev, "campos");
  Tensor bgc = f32c(bg, dev, "bg");
  if (bgc.numel() == 3 && B > 1) bgc = bgc.reshape({1, 3}).expand({B, 3}).contiguous();
  r.bg = bgc;
  if (r.bg.numel() != 3 * B || r.vm.numel() != 16 * B || r.pm.numel() != 16 * B || r.cp.numel() != 3 * B)
    throw std::runtime_error("bg/campos must have 3 elements (per view), viewmatrix/projmatrix 16");
  r.s.resize(B);
  for (int64_t b = 0; b < B; ++b) {
    hgs_settings& s = r.s[b];
    s.image_height = (int32_t)H;
    s.image_width = (int32_t)W;
    s.tanfovx = (float)tanfovx[b];
    s.tanfovy = (float)tanfovy[b];
    s.bg = r.bg.data_ptr<float>() + 3 * b;
    s.scale_modifier = (float)scale_modifier;
    s.viewmatrix = r.vm.data_ptr<float>() + 16 * b;
    s.projmatrix = r.pm.data_ptr<float>() + 16 * b;
    s.sh_degree = (int32_t)sh_degree;
    s.campos = r.cp.data_ptr<float>() + 3 * b;
    s.prefiltered = prefiltered ? 1 : 0;
    s.debug = debug ? 1 : 0;
  }
  return r;
}

void check_rc(int rc, const char* what) {
  if (rc == HGS_ESHAPE)
    throw std::runtime_error("inconsistent optional inputs (shs/colors_precomp, scales+rotations/cov3D_precomp)");
  if (rc != HGS_OK) throw std::runtime_error(std::string("libhgs_rast: ") + what + " failed with code " + std::to_string(rc));
}

void need_numel(const Tensor& t, int64_t n, const char* name, const char* shape) {
  if (t.numel() != n)
    throw std::runtime_error(std::string(name) + " must have dimensions " + shape + " (got " + std::to_string(t.numel()) +
                             " elements, expected " + std::to_string(n) + ")");
}

// What the backward call needs.  The plan stays alive as long as the autograd node does, so the
// backward can run more than once (retain_graph=True, torch.autograd.grad per loss term) like
// upstream's Python autograd.Function; gradient tensors are allocated per backward call.
struct BwdPlan : torch::CustomClassHolder {
  Settings settings;
  Tensor work, work2;                 // [geom | img | bin | rows] (work2: bin | rows after a retry)
  char *geom = nullptr, *bin = nullptr, *img = nullptr, *rows = nullptr;
  int64_t cap = 0;
  hgs_status status{};
  // the pinned status slot of the forward call and its issue number: the blend forward writes num_pairs there once the
  // sort has run; backward() sizes its pair rows by it while the slot is known not to have been handed out again
  const hgs_status* slot = nullptr;
  int64_t slot_issue = 0;
  int32_t B = 1, P = 0, M = 0, act = 0;
  bool batched = false;
  bool has_sh = false, has_cp = false, has_sr = false, has_cv = false;
  std::vector<int64_t> opac_sizes;
  // gradient tensors of the FIRST backward call, allocated by forward() while it waits for the device-side status
  // (host time that is otherwise idle; in backward() the same allocations sit on the step's critical host path)
  std::vector<Tensor> pre_grads;
  void* pre_stream = nullptr;

  void alloc_grads(std::vector<Tensor>& g, const c10::Device& dev) const {
    const auto fopt = at::TensorOptions().dtype(at::kFloat).device(dev);
    g.assign(8, Tensor());
    g[0] = at::empty({(int64_t)P, 3}, fopt);                                                             // means3D
    g[1] = batched ? at::empty({(int64_t)B, (int64_t)P, 3}, fopt) : at::empty({(int64_t)P, 3}, fopt);   // means2D
    if (has_sh) g[2] = at::empty({(int64_t)P, (int64_t)M, 3}, fopt);
    if (has_cp) g[3] = at::empty({(int64_t)P, 3}, fopt);
    g[4] = at::empty(opac_sizes, fopt);
    if (has_sr) { g[5] = at::empty({(int64_t)P, 3}, fopt); g[6] = at::empty({(int64_t)P, 4}, fopt); }
    if (has_cv) g[7] = at::empty({(int64_t)P, 6}, fopt);
  }
};

// Packed backward (view_parallel.py): while a request is open, a backward whose inputs are the SH / scale / rotation
// configuration writes ONE (P, 15 + 3M) pack (hgs_backward_batch_packed) - the tensor the rank sends - and hands autograd
// strided views of it; `take_packed()` collects the pack.  Process-wide, not thread-local: torch's engine runs a
// CPU-initiated backward of one device on that device's worker thread, not on the thread that called autograd.grad, so
// the request is read through an atomic and the pack is kept per process.  Requests nest (an inner exit leaves the outer
// request open, with its own slot); every rasterizer backward that runs while one is open is counted, and `take_packed()`
// hands out the pack only when exactly ONE backward ran since the slot was last cleared - a graph with two rasterizer
// nodes (or one eligible and one not) has no single pack that holds its gradients.
std::atomic<int> g_pack_request{0};
std::mutex g_pack_mu;
Tensor g_last_pack;
int64_t g_pack_backwards = 0;       // rasterizer backwards since the slot was last cleared (under g_pack_mu)
std::vector<std::pair<Tensor, int64_t>> g_pack_saved;     // slot + count of each enclosing request (under g_pack_mu)

struct Rasterize : public torch::autograd::Function<Rasterize> {
  // 22 arguments after ctx (backward returns one slot per argument).  `tanfov` is a CPU double
  // tensor [2][B] (x row, y row); `batch` = 0 for the single-view API, else the number of views;
  // `act` = HGS_ACT_* bits (raw parameters in, activations fused into the per-Gaussian kernels) and HGS_ANTIALIAS; the
  // plan keeps them for the backward (whichever it runs: the bit must reach it as it reached the forward).
  static variable_list forward(AutogradContext* ctx, const Tensor& means3D, const Tensor& means2D,
                               const Tensor& sh, const Tensor& colors_precomp, const Tensor& opacities,
                               const Tensor& scales, const Tensor& rotations, const Tensor& cov3D,
                               const Tensor& bg, const Tensor& viewmatrix, const Tensor& projmatrix,
                               const Tensor& campos, const Tensor& tanfov, int64_t H, int64_t W,
                               double scale_modifier, int64_t sh_degree, bool prefiltered, bool debug,
                               bool want_grad, int64_t batch, int64_t act_in) {
    // bit 16 of `act` is the binding's own (never handed to the library): `means2D` is UNINITIALISED storage that the
    // forward's per-Gaussian kernel zero-fills (ABI v16: hgs_forward_batch_act_leaf) - what renderer.render() passes
    // instead of launching torch.zeros
    const bool zero_leaf = ((act_in >> 16) & 1) != 0;
    const int64_t act = act_in & 0xffff;
    const auto th0 = std::chrono::steady_clock::now();
    const c10::Device dev = means3D.device();
    if (!dev.is_cuda())
      throw std::runtime_error("humangaussian_amd: tensors must live on a HIP device (torch device type 'cuda'); "
                               "there is no CPU path");
    const bool batched = batch > 0;
    const int64_t B = batched ? batch : 1;
    const int64_t P = means3D.size(0);
    if (P != 0 && (means3D.dim() != 2 || means3D.size(1) != 3))
      throw std::runtime_error("means3D must have dimensions (num_points, 3)");
    if (tanfov.device().is_cuda() || tanfov.scalar_type() != at::kDouble || tanfov.numel() != 2 * B || !tanfov.is_contiguous())
      throw std::runtime_error("tanfov must be a contiguous CPU double tensor of shape (2, views)");
    DeviceSwitch guard(dev.index());

    auto plan = c10::make_intrusive<BwdPlan>();
    const double* tf = tanfov.data_ptr<double>();
    plan->settings = make_settings(bg, viewmatrix, projmatrix, campos, B, H, W, tf, tf + B, scale_modifier, sh_degree,
                                   prefiltered, debug, dev);
    const Tensor m3 = f32c(means3D, dev, "means3D");
    const bool has_sh = sh.defined() && sh.numel() > 0, has_cp = colors_precomp.defined() && colors_precomp.numel() > 0;
    const bool has_sc = scales.defined() && scales.numel() > 0, has_ro = rotations.defined() && rotations.numel() > 0;
    const bool has_cv = cov3D.defined() && cov3D.numel() > 0;
    const Tensor sh_ = has_sh ? f32c(sh, dev, "shs") : Tensor();
    const Tensor cp_ = has_cp ? f32c(colors_precomp, dev, "colors_precomp") : Tensor();
    const Tensor sc_ = has_sc ? f32c(scales, dev, "scales") : Tensor();
    const Tensor ro_ = has_ro ? f32c(rotations, dev, "rotations") : Tensor();
    const Tensor cv_ = has_cv ? f32c(cov3D, dev, "cov3D_precomp") : Tensor();
    const Tensor op_ = f32c(opacities, dev, "opacities");
    if (has_sh && (sh_.dim() != 3 || sh_.size(0) != P || sh_.size(2) != 3))
      throw std::runtime_error("shs must have dimensions (num_points, M, 3)");
    const int32_t M = has_sh ? (int32_t)sh_.size(1) : 0;
    // the kernels index every per-Gaussian tensor by P: a stale tensor (captured before a
    // densification / pruning step) must fail here, not read out of bounds on the device
    need_numel(op_, P, "opacities", "(num_points, 1)");
    if (has_cp) need_numel(cp_, 3 * P, "colors_precomp", "(num_points, 3)");
    if (has_sc) need_numel(sc_, 3 * P, "scales", "(num_points, 3)");
    if (has_ro) need_numel(ro_, 4 * P, "rotations", "(num_points, 4)");
    if (has_cv) need_numel(cv_, 6 * P, "cov3D_precomp", "(num_points, 6)");

    const auto fopt = at::TensorOptions().dtype(at::kFloat).device(dev);
    Tensor color, depth, alpha, radii;
    if (batched) {
      color = at::empty({B, 3, H, W}, fopt); depth = at::empty({B, 1, H, W}, fopt); alpha = at::empty({B, 1, H, W}, fopt);
      radii = at::empty({B, P}, fopt.dtype(at::kInt));
    } else {
      color = at::empty({3, H, W}, fopt); depth = at::empty({1, H, W}, fopt); alpha = at::empty({1, H, W}, fopt);
      radii = at::empty({P}, fopt.dtype(at::kInt));
    }

    float* leaf_ptr = nullptr;
    if (zero_leaf && means2D.defined() && means2D.numel() > 0) {
      if (means2D.numel() != B * P * 3) throw std::runtime_error("means2D must have (views x) num_points x 3 elements");
      if (means2D.device() == dev && means2D.scalar_type() == at::kFloat && means2D.is_contiguous()) {
        leaf_ptr = static_cast<float*>(means2D.data_ptr());
      } else {                       // (a leaf the kernel cannot write: filled the ordinary way)
        at::NoGradGuard ng;
        const_cast<Tensor&>(means2D).zero_();
      }
    }

    DevState& st = state_for(dev.index());
    std::lock_guard<std::mutex> lk(st.mu);
    hipStream_t stream = c10::hip::getCurrentHIPStream(dev.index()).stream();
    Estimate& est = st.est[std::make_tuple(B, H, W)];
    int64_t cap = P > 0 ? (est.capacity > 0 ? est.capacity : round_capacity(3 * P * B)) : 0;
    int32_t hint = (int32_t)est.tile_hint;
    // one allocation for the four opaque regions [geom | img | bin | backward rows] (the fork keeps
    // three such byte tensors for its backward); a capacity retry re-allocates only the last two
    const int64_t g_sz = al256(hgs_geom_bytes_batch((int32_t)B, (int32_t)P, (int32_t)H, (int32_t)W));
    const int64_t i_sz = al256(hgs_img_bytes_batch((int32_t)B, (int32_t)H, (int32_t)W));
    // (the backward's pair rows - 16 x 40 B per entry - are allocated by backward() for its own duration: they would
    // otherwise be held by every view of a step until its backward runs)
    int64_t b_sz = al256(hgs_bin_bytes(cap));
    const int64_t s_sz = 0;
    const auto bopt = at::TensorOptions().dtype(at::kByte).device(dev);
    plan->work = at::empty({g_sz + i_sz + b_sz + s_sz}, bopt);
    char* base = static_cast<char*>(plan->work.data_ptr());
    plan->geom = base;
    plan->img = base + g_sz;
    plan->bin = base + g_sz + i_sz;
    plan->rows = base + g_sz + i_sz + b_sz;

    hgs_status h{};
    int attempt = 0;
    for (; attempt < 4; ++attempt) {
      const int slot = st.ring_pos;
      st.ring_pos = (st.ring_pos + 1) % RING;
      st.ring_issued += 1;
      plan->slot = &st.ring[slot];
      plan->slot_issue = st.ring_issued;
      // The library stores the status into this pinned slot from the fill launch and sets reserved[2] = 1 LAST (behind a
      // system-scope fence): the host polls that word.  (An event recorded behind the fill stage cost the GPU ~6 us of
      // idle time per forward: the record is a barrier packet with a system-scope release in the middle of the chain.)
      volatile uint32_t* ready = &st.ring[slot].reserved[2];
      *ready = 0u;
      std::atomic_thread_fence(std::memory_order_seq_cst);
      const auto th1 = std::chrono::steady_clock::now();
      if (attempt == 0) st.host_ns[0] += std::chrono::duration_cast<std::chrono::nanoseconds>(th1 - th0).count();
      const int rc = hgs_forward_batch_act_leaf(plan->settings.s.data(), (int32_t)B, (int32_t)P, M, fptr(m3), fptr(sh_), fptr(cp_),
                                                fptr(op_), fptr(sc_), fptr(ro_), fptr(cv_), fptr_mut(color), fptr_mut(depth),
                                                fptr_mut(alpha), P > 0 ? radii.data_ptr<int32_t>() : nullptr, plan->geom,
                                                plan->bin, cap, plan->img, want_grad ? 1 : 0, hint, &st.ring[slot], /*mapped=*/1,
                                                /*status_event=*/nullptr, g_stage_fwd.empty() ? nullptr : g_stage_fwd.data(),
                                                (int32_t)act, leaf_ptr, stream);
      check_rc(rc, "hgs_forward_batch");
      const auto th2 = std::chrono::steady_clock::now();
      st.host_ns[1] += std::chrono::duration_cast<std::chrono::nanoseconds>(th2 - th1).count();
      // `debug=True` is upstream's switch for surfacing device errors at the call that caused
      // them (std::runtime_error): synchronise and report
      if (debug) hip_ok(hipStreamSynchronize(stream), "device error in the rasterizer forward (debug=True)");
      // Host work that does not depend on the status goes HERE, in the shadow of the wait below (with an idle GPU
      // that wait is the ~25 us the first two kernels take): the autograd bookkeeping and the gradient tensors of
      // the backward call.  (Measured: a step is ~172 us of kernels and ~170 us of host work; whatever sits behind
      // the wait is on the critical path whenever the host is the slower of the two.)
      if (attempt == 0 && want_grad) {
        plan->B = (int32_t)B; plan->P = (int32_t)P; plan->M = M;
        plan->batched = batched;
        plan->act = (int32_t)act;
        plan->has_sh = has_sh; plan->has_cp = has_cp; plan->has_sr = has_sc; plan->has_cv = has_cv;
        plan->opac_sizes = opacities.sizes().vec();
        // inputs and outputs go through save_for_backward (version checks: the backward reads the
        // forward's outputs, so they must not be modified in place before backward()); the opaque
        // work buffers ride in the plan
        variable_list saved = {m3, op_, radii, color, depth, alpha};
        for (const Tensor* t : {&sh_, &cp_, &sc_, &ro_, &cv_})
          if (t->defined()) saved.push_back(*t);
        ctx->save_for_backward(saved);
        plan->alloc_grads(plan->pre_grads, dev);
        plan->pre_stream = (void*)stream;
      }
      // One host wait per forward, like upstream's blocking read of num_rendered - but only for the status: sort and
      // blend are already enqueued and keep the GPU busy while the host goes on to autograd and the backward launch.
      const auto tw = std::chrono::steady_clock::now();
      st.host_ns[2] += std::chrono::duration_cast<std::chrono::nanoseconds>(tw - th2).count();
      for (uint64_t spins = 0; *ready == 0u; ++spins) {
        if ((spins & 0x3ff) == 0x3ff) {
          if (std::chrono::steady_clock::now() - tw > std::chrono::seconds(2)) {       // (a device error: surface it)
            hip_ok(hipStreamSynchronize(stream), "rasterizer forward");
            if (*ready == 0u) throw std::runtime_error("libhgs_rast: the forward finished without publishing its status");
            break;
          }
          std::this_thread::yield();
        }
      }
      std::atomic_thread_fence(std::memory_order_seq_cst);
      const int64_t waited = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - tw).count();
      st.wait_ns += waited;
      st.host_ns[3] += waited;
      h = st.ring[slot];
      if (!h.overflow) break;
      st.retries += 1;
      if (h.overflow & 1u) {                    // R exceeded the capacity: grow, re-run
        cap = round_capacity((int64_t)(h.num_rendered * 1.25) + 1);
        b_sz = al256(hgs_bin_bytes(cap));
        plan->work2 = at::empty({b_sz + s_sz}, bopt);
        plan->bin = static_cast<char*>(plan->work2.data_ptr());
        plan->rows = plan->bin + b_sz;
      }
      if (h.overflow & 2u) hint = 0;            // a tile list outgrew the hint
    }
    if (attempt == 4) throw std::runtime_error("libhgs_rast: entry capacity did not converge");
    st.calls += 1;
    st.max_R = h.num_rendered;
    st.max_tile = h.reserved[1];
    st.last_capacity = cap;
    st.last_hint = hint;
    if (P > 0) {
      // decaying maxima: follow the workload down slowly, up at once
      est.capacity = std::max<int64_t>(round_capacity((int64_t)(h.num_rendered * 1.25) + 1),
                                       est.capacity > 0 ? round_capacity((int64_t)(est.capacity * 0.9)) : 0);
      est.tile_hint = std::max<int64_t>(std::max<int64_t>(1024, (int64_t)(h.reserved[1] * 1.5) + 64),
                                        (int64_t)(est.tile_hint * 0.9));
    }
    ctx->set_materialize_grads(false);
    if (want_grad) {
      plan->cap = cap;
      plan->status = h;
      ctx->saved_data["plan"] = c10::IValue::make_capsule(plan);
    }
    ctx->mark_non_differentiable({radii});
    st.host_ns[4] += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - th0).count();   // whole forward()
    return {color, radii, depth, alpha};
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    const auto tb0 = std::chrono::steady_clock::now();
    auto it = ctx->saved_data.find("plan");
    if (it == ctx->saved_data.end() || it->second.isNone())
      throw std::runtime_error("humangaussian_amd: the rasterizer's backward state is gone (the forward ran without "
                               "gradient tracking)");
    auto holder = it->second.toCapsule();
    BwdPlan* plan = static_cast<BwdPlan*>(holder.get());
    const auto saved = ctx->get_saved_variables();
    const Tensor &m3 = saved[0], &op_ = saved[1], &radii = saved[2], &color = saved[3], &depth = saved[4], &alpha = saved[5];
    size_t k = 6;
    const Tensor sh_ = plan->has_sh ? saved[k++] : Tensor();
    const Tensor cp_ = plan->has_cp ? saved[k++] : Tensor();
    const Tensor sc_ = plan->has_sr ? saved[k++] : Tensor();
    const Tensor ro_ = plan->has_sr ? saved[k++] : Tensor();
    const Tensor cv_ = plan->has_cv ? saved[k++] : Tensor();
    const c10::Device dev = m3.device();
    DeviceSwitch guard(dev.index());
    const Tensor gc = grads[0].defined() ? f32c(grads[0], dev, "grad_color") : Tensor();
    const Tensor gd = grads[2].defined() ? f32c(grads[2], dev, "grad_depth") : Tensor();
    const Tensor ga = grads[3].defined() ? f32c(grads[3], dev, "grad_alpha") : Tensor();
    hipStream_t stream = c10::hip::getCurrentHIPStream(dev.index()).stream();
    std::vector<Tensor> g;
    if (!plan->pre_grads.empty() && plan->pre_stream == (void*)stream) g = std::move(plan->pre_grads);
    plan->pre_grads.clear();
    if (g.empty()) plan->alloc_grads(g, dev);
    Tensor &d_means3D = g[0], &d_means2D = g[1], &d_sh = g[2], &d_cp = g[3], &d_opac = g[4], &d_sc = g[5], &d_ro = g[6], &d_cv = g[7];
    // pair rows: 16 per entry in the worst case, ~4.4 on an avatar - counted once the forward's sort has run (the
    // blend forward then publishes hgs_status.num_pairs into the call's pinned slot; nothing is waited for here)
    int64_t pairs = 0;
    {
      DevState& st = state_for(dev.index());
      std::lock_guard<std::mutex> lk(st.mu);
      if (plan->slot && st.ring_issued - plan->slot_issue < RING - 1)
        pairs = (int64_t)*reinterpret_cast<const volatile uint32_t*>(&plan->slot->num_pairs);
      st.last_pairs = pairs;
      st.last_scratch = al256(hgs_bwd_scratch_bytes_pairs((int64_t)plan->status.num_rendered, pairs));
    }
    Tensor scratch = at::empty({al256(hgs_bwd_scratch_bytes_pairs((int64_t)plan->status.num_rendered, pairs))},
                               at::TensorOptions().dtype(at::kByte).device(dev));
    plan->rows = static_cast<char*>(scratch.data_ptr());
    // tell the library what the scratch holds: its kernels check the count against the one the sort left on the device and
    // write nothing (NaN gradients) if the slot delivered a stale number (hgs_rast.h: hgs_backward)
    plan->status.num_pairs = (uint32_t)pairs;
    const auto tb1 = std::chrono::steady_clock::now();
    const bool requested = g_pack_request.load(std::memory_order_relaxed) > 0;
    if (requested) {                          // (eligible or not: `take_packed` needs to know how many nodes there were)
      std::lock_guard<std::mutex> lk(g_pack_mu);
      ++g_pack_backwards;
    }
    const bool packed = requested && plan->has_sh && plan->has_sr && !plan->has_cp && !plan->has_cv && plan->M >= 1 &&
                        plan->P > 0;
    if (packed) {
      const int64_t P = plan->P, M = plan->M, F = 15 + 3 * M;
      Tensor pack = at::empty({P, F}, at::TensorOptions().dtype(at::kFloat).device(dev));
      const int rc = hgs_backward_batch_packed(
          plan->settings.s.data(), plan->B, plan->P, plan->M, fptr(m3), fptr(sh_), fptr(op_), fptr(sc_), fptr(ro_),
          radii.data_ptr<int32_t>(), fptr(color), fptr(depth), fptr(alpha), fptr(gc), fptr(gd), fptr(ga), plan->geom, plan->bin,
          plan->img, &plan->status, plan->cap, plan->rows, pack.data_ptr<float>(),
          plan->batched ? fptr_mut(d_means2D) : nullptr, g_stage_bwd.empty() ? nullptr : g_stage_bwd.data(), plan->act, stream);
      check_rc(rc, "hgs_backward_batch_packed");
      variable_list out(22);
      out[0] = pack.as_strided({P, 3}, {F, 1}, 0);
      out[1] = plan->batched ? d_means2D : pack.as_strided({P, 3}, {F, 1}, 3);
      out[2] = pack.as_strided({P, M, 3}, {F, 3, 1}, 6);
      {
        std::vector<int64_t> os = plan->opac_sizes, ostr(plan->opac_sizes.size(), 1);
        if (!ostr.empty()) ostr[0] = F;
        out[4] = pack.as_strided(os, ostr, 6 + 3 * M);
      }
      out[5] = pack.as_strided({P, 3}, {F, 1}, 7 + 3 * M);
      out[6] = pack.as_strided({P, 4}, {F, 1}, 10 + 3 * M);
      {
        std::lock_guard<std::mutex> lk(g_pack_mu);
        g_last_pack = pack;
      }
      DevState& st = state_for(dev.index());
      const auto tb2 = std::chrono::steady_clock::now();
      st.host_ns[5] += std::chrono::duration_cast<std::chrono::nanoseconds>(tb1 - tb0).count();
      st.host_ns[6] += std::chrono::duration_cast<std::chrono::nanoseconds>(tb2 - tb1).count();
      st.host_ns[7] += std::chrono::duration_cast<std::chrono::nanoseconds>(tb2 - tb0).count();
      return out;
    }
    const int rc = hgs_backward_batch_act(
        plan->settings.s.data(), plan->B, plan->P, plan->M, fptr(m3), fptr(sh_), fptr(cp_), fptr(op_), fptr(sc_), fptr(ro_),
        fptr(cv_), plan->P > 0 ? radii.data_ptr<int32_t>() : nullptr, fptr(color), fptr(depth), fptr(alpha), fptr(gc),
        fptr(gd), fptr(ga), plan->geom, plan->bin, plan->img, &plan->status, plan->cap, plan->rows, fptr_mut(d_means3D),
        fptr_mut(d_means2D), fptr_mut(d_sh), fptr_mut(d_cp), fptr_mut(d_opac), fptr_mut(d_sc), fptr_mut(d_ro),
        fptr_mut(d_cv), g_stage_bwd.empty() ? nullptr : g_stage_bwd.data(), plan->act, stream);
    check_rc(rc, "hgs_backward_batch");
    const auto tb2 = std::chrono::steady_clock::now();
    if (plan->settings.s[0].debug) hip_ok(hipStreamSynchronize(stream), "device error in the rasterizer backward (debug=True)");
    variable_list out(22);
    out[0] = d_means3D; out[1] = d_means2D; out[2] = d_sh; out[3] = d_cp;
    out[4] = d_opac; out[5] = d_sc; out[6] = d_ro; out[7] = d_cv;
    {
      DevState& st = state_for(dev.index());
      st.host_ns[5] += std::chrono::duration_cast<std::chrono::nanoseconds>(tb1 - tb0).count();
      st.host_ns[6] += std::chrono::duration_cast<std::chrono::nanoseconds>(tb2 - tb1).count();
      st.host_ns[7] += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - tb0).count();   // whole backward()
    }
    return out;
  }
};

// None optionals travel through autograd as one shared empty tensor (upstream does the same:
// "None inputs become empty tensors"); undefined tensors are not valid apply() inputs.
Tensor opt(const c10::optional<Tensor>& t) {
  static const Tensor empty = at::empty({0}, at::TensorOptions().dtype(at::kFloat));
  return t.has_value() ? *t : empty;
}

Tensor tanfov_tensor(const std::vector<double>& x, const std::vector<double>& y) {
  if (x.size() != y.size() || x.empty()) throw std::runtime_error("tanfovx / tanfovy: one value per view");
  Tensor t = at::empty({2, (int64_t)x.size()}, at::TensorOptions().dtype(at::kDouble));
  double* d = t.data_ptr<double>();
  for (size_t i = 0; i < x.size(); ++i) { d[i] = x[i]; d[x.size() + i] = y[i]; }
  return t;
}

// single view: the signature of upstream's _C.rasterize_gaussians call, plus the library's flag bits (HGS_ANTIALIAS;
// 0 = upstream's behaviour)
std::vector<Tensor> rasterize(const Tensor& means3D, const Tensor& means2D, const c10::optional<Tensor>& sh,
                              const c10::optional<Tensor>& colors_precomp, const Tensor& opacities,
                              const c10::optional<Tensor>& scales, const c10::optional<Tensor>& rotations,
                              const c10::optional<Tensor>& cov3D, const Tensor& bg, const Tensor& viewmatrix,
                              const Tensor& projmatrix, const Tensor& campos, int64_t H, int64_t W, double tanfovx,
                              double tanfovy, double scale_modifier, int64_t sh_degree, bool prefiltered, bool debug,
                              bool want_grad, bool zero_means2D, int64_t activation_flags) {
  if (activation_flags & ~(int64_t)0xffff) throw std::runtime_error("rasterize: unknown activation_flags bits");
  return Rasterize::apply(means3D, means2D, opt(sh), opt(colors_precomp), opacities, opt(scales), opt(rotations),
                          opt(cov3D), bg, viewmatrix, projmatrix, campos, tanfov_tensor({tanfovx}, {tanfovy}), H, W,
                          scale_modifier, sh_degree, prefiltered, debug, want_grad, (int64_t)0,
                          activation_flags | (int64_t)(zero_means2D ? (1 << 16) : 0));
}

// B views in one launch set: bg (3) or (B,3), viewmatrix / projmatrix (B,4,4), campos (B,3), means2D (B,P,3);
// returns color (B,3,H,W), radii (B,P), depth (B,1,H,W), alpha (B,1,H,W)
std::vector<Tensor> rasterize_batch(const Tensor& means3D, const Tensor& means2D, const c10::optional<Tensor>& sh,
                                    const c10::optional<Tensor>& colors_precomp, const Tensor& opacities,
                                    const c10::optional<Tensor>& scales, const c10::optional<Tensor>& rotations,
                                    const c10::optional<Tensor>& cov3D, const Tensor& bg, const Tensor& viewmatrix,
                                    const Tensor& projmatrix, const Tensor& campos, int64_t H, int64_t W,
                                    const std::vector<double>& tanfovx, const std::vector<double>& tanfovy,
                                    double scale_modifier, int64_t sh_degree, bool prefiltered, bool debug,
                                    bool want_grad, int64_t activation_flags) {
  const int64_t B = (int64_t)tanfovx.size();
  if (means2D.defined() && means2D.numel() > 0 && means2D.numel() != B * means3D.size(0) * 3)
    throw std::runtime_error("means2D must have dimensions (views, num_points, 3) for a batched call");
  return Rasterize::apply(means3D, means2D, opt(sh), opt(colors_precomp), opacities, opt(scales), opt(rotations),
                          opt(cov3D), bg, viewmatrix, projmatrix, campos, tanfov_tensor(tanfovx, tanfovy), H, W,
                          scale_modifier, sh_degree, prefiltered, debug, want_grad, B, activation_flags);
}

Tensor mark_visible(const Tensor& positions, const Tensor& bg, const Tensor& viewmatrix, const Tensor& projmatrix,
                    const Tensor& campos, int64_t H, int64_t W, double tanfovx, double tanfovy, double scale_modifier,
                    int64_t sh_degree, bool prefiltered, bool debug) {
  at::NoGradGuard ng;
  const c10::Device dev = positions.device();
  if (!dev.is_cuda()) throw std::runtime_error("humangaussian_amd: tensors must live on a HIP device");
  DeviceSwitch guard(dev.index());
  Settings s = make_settings(bg, viewmatrix, projmatrix, campos, 1, H, W, &tanfovx, &tanfovy, scale_modifier, sh_degree,
                             prefiltered, debug, dev);
  const Tensor pos = f32c(positions, dev, "positions");
  const int64_t P = pos.size(0);
  Tensor present = at::zeros({P}, at::TensorOptions().dtype(at::kByte).device(dev));
  if (P > 0) {
    const int rc = hgs_mark_visible(s.s.data(), (int32_t)P, pos.data_ptr<float>(), present.data_ptr<uint8_t>(),
                                    c10::hip::getCurrentHIPStream(dev.index()).stream());
    check_rc(rc, "hgs_mark_visible");
  }
  return present.to(at::kBool);
}

// replaces simple_knn._C.distCUDA2: mean squared distance to the 3 nearest neighbours
Tensor knn_mean_dist2(const Tensor& points, bool brute_force) {
  at::NoGradGuard ng;
  const c10::Device dev = points.device();
  if (!dev.is_cuda()) throw std::runtime_error("humangaussian_amd: tensors must live on a HIP device");
  if (points.dim() != 2 || points.size(1) != 3) throw std::runtime_error("points must have dimensions (num_points, 3)");
  DeviceSwitch guard(dev.index());
  const Tensor pts = f32c(points, dev, "points");
  const int64_t P = pts.size(0);
  Tensor out = at::empty({P}, at::TensorOptions().dtype(at::kFloat).device(dev));
  if (P > 0x7fffffffll / 4) throw std::runtime_error("too many points");
  if (P > 0 && brute_force) {
    const int rc = hgs_knn_mean_dist2((int32_t)P, pts.data_ptr<float>(), out.data_ptr<float>(),
                                      c10::hip::getCurrentHIPStream(dev.index()).stream());
    check_rc(rc, "hgs_knn_mean_dist2");
  } else if (P > 0) {      // the grid form (near-linear); its scratch lives for the duration of the call's stream work
    Tensor scratch = at::empty({(int64_t)hgs_knn_scratch_bytes((int32_t)P)}, at::TensorOptions().dtype(at::kByte).device(dev));
    const int rc = hgs_knn_mean_dist2_grid((int32_t)P, pts.data_ptr<float>(), out.data_ptr<float>(), scratch.data_ptr(),
                                           c10::hip::getCurrentHIPStream(dev.index()).stream());
    check_rc(rc, "hgs_knn_mean_dist2_grid");
  }
  return out;
}

// one rank's (P, 15 + 3M) pack for the view-parallel all-gather
Tensor pack_view_contribution(const Tensor& g_means3D, const Tensor& g_means2D, const Tensor& g_sh,
                              const Tensor& g_opac, const Tensor& g_scales, const Tensor& g_rot,
                              const Tensor& radii) {
  at::NoGradGuard ng;
  const c10::Device dev = g_means3D.device();
  if (!dev.is_cuda()) throw std::runtime_error("humangaussian_amd: tensors must live on a HIP device");
  DeviceSwitch guard(dev.index());
  const int64_t P = g_means3D.size(0);
  const Tensor a = f32c(g_means3D, dev, "means3D grad"), b = f32c(g_means2D, dev, "means2D grad");
  const Tensor c = f32c(g_sh, dev, "sh grad"), d = f32c(g_opac, dev, "opacity grad");
  const Tensor e = f32c(g_scales, dev, "scales grad"), f = f32c(g_rot, dev, "rotations grad");
  if (radii.device() != dev || radii.scalar_type() != at::kInt) throw std::runtime_error("radii must be int32 on the same device");
  const Tensor r = radii.contiguous();
  const int64_t M = P > 0 ? c.numel() / (3 * P) : 0;
  if (a.numel() != 3 * P || b.numel() != 3 * P || c.numel() != 3 * M * P || d.numel() != P || e.numel() != 3 * P ||
      f.numel() != 4 * P || r.numel() != P)
    throw std::runtime_error("pack_view_contribution: inconsistent shapes");
  Tensor out = at::empty({P, 15 + 3 * M}, a.options());
  const int rc = hgs_pack_view_contribution((int32_t)P, (int32_t)M, fptr(a), fptr(b), fptr(c), fptr(d), fptr(e), fptr(f),
                                            P > 0 ? r.data_ptr<int32_t>() : nullptr, fptr_mut(out),
                                            c10::hip::getCurrentHIPStream(dev.index()).stream());
  check_rc(rc, "hgs_pack_view_contribution");
  return out;
}

// view-parallel reduction of the all-gathered packs: (world, P, F) [+ the running total (P, F) of the step's earlier
// collectives] -> (P, F), one left-to-right chain
Tensor reduce_view_packs(const Tensor& gathered, const c10::optional<Tensor>& acc_in) {
  at::NoGradGuard ng;
  const c10::Device dev = gathered.device();
  if (!dev.is_cuda()) throw std::runtime_error("humangaussian_amd: tensors must live on a HIP device");
  if (gathered.dim() != 3) throw std::runtime_error("gathered packs must have dimensions (world, num_points, F)");
  DeviceSwitch guard(dev.index());
  const Tensor g = f32c(gathered, dev, "gathered");
  Tensor a;
  if (acc_in.has_value() && acc_in->defined()) {
    a = f32c(*acc_in, dev, "running total");
    if (a.numel() != g.size(1) * g.size(2)) throw std::runtime_error("running total must have dimensions (num_points, F)");
  }
  Tensor out = at::empty({g.size(1), g.size(2)}, g.options());
  const int rc = hgs_reduce_view_packs_acc((int32_t)g.size(0), g.size(1), (int32_t)g.size(2), g.data_ptr<float>(),
                                           a.defined() ? a.data_ptr<float>() : nullptr, out.data_ptr<float>(),
                                           c10::hip::getCurrentHIPStream(dev.index()).stream());
  check_rc(rc, "hgs_reduce_view_packs_acc");
  return out;
}

// open (on = true) or close one packed-gradients request.  Opening saves the enclosing request's slot and count and
// starts empty; closing restores them: an inner request neither ends the outer one nor hands its pack to it (a pack the
// inner request did not take is dropped).
void set_packed_backward(bool on) {
  std::lock_guard<std::mutex> lk(g_pack_mu);
  if (on) {
    g_pack_saved.emplace_back(g_last_pack, g_pack_backwards);
    g_last_pack = Tensor();
    g_pack_backwards = 0;
  } else {
    if (g_pack_saved.empty()) return;               // (unbalanced close: nothing is open)
    g_last_pack = g_pack_saved.back().first;
    g_pack_backwards = g_pack_saved.back().second;
    g_pack_saved.pop_back();
  }
  g_pack_request.store((int)g_pack_saved.size(), std::memory_order_relaxed);
}

// the pack of the one packed backward since the slot was last cleared, once (None if the backward was not eligible -
// colours / covariances precomputed -, if none ran, or if more than one rasterizer backward ran: the caller then packs
// the six tensors itself)
c10::optional<Tensor> take_packed() {
  std::lock_guard<std::mutex> lk(g_pack_mu);
  Tensor t = g_last_pack;
  const int64_t n = g_pack_backwards;
  g_last_pack = Tensor();
  g_pack_backwards = 0;
  if (!t.defined() || n != 1) return c10::nullopt;
  return t;
}

// the LAST reduction of a view-parallel step with the unpack fused in: (world, P, 15 + 3M) [+ running total (P, F)] ->
// [means3D (P,3), means2D (P,3), sh (P,M,3), opacity (P,1), scales (P,3), rotations (P,4), radii (P,) int32]
std::vector<Tensor> reduce_view_packs_unpack(const Tensor& gathered, const c10::optional<Tensor>& acc_in) {
  at::NoGradGuard ng;
  const c10::Device dev = gathered.device();
  if (!dev.is_cuda()) throw std::runtime_error("humangaussian_amd: tensors must live on a HIP device");
  if (gathered.dim() != 3 || gathered.size(2) < 15 || (gathered.size(2) - 15) % 3)
    throw std::runtime_error("gathered packs must have dimensions (world, num_points, 15 + 3 M)");
  DeviceSwitch guard(dev.index());
  const Tensor g = f32c(gathered, dev, "gathered");
  const int64_t P = g.size(1), F = g.size(2), M = (F - 15) / 3;
  Tensor a;
  if (acc_in.has_value() && acc_in->defined()) {
    a = f32c(*acc_in, dev, "running total");
    if (a.numel() != P * F) throw std::runtime_error("running total must have dimensions (num_points, F)");
  }
  const auto fopt = g.options();
  Tensor m3 = at::empty({P, 3}, fopt), m2 = at::empty({P, 3}, fopt), sh = at::empty({P, M, 3}, fopt);
  Tensor op = at::empty({P, 1}, fopt), sc = at::empty({P, 3}, fopt), ro = at::empty({P, 4}, fopt);
  Tensor radii = at::empty({P}, fopt.dtype(at::kInt));
  const int rc = hgs_reduce_view_packs_unpack((int32_t)g.size(0), P, (int32_t)M, g.data_ptr<float>(),
                                              a.defined() ? a.data_ptr<float>() : nullptr, fptr_mut(m3), fptr_mut(m2),
                                              fptr_mut(sh), fptr_mut(op), fptr_mut(sc), fptr_mut(ro),
                                              P > 0 ? radii.data_ptr<int32_t>() : nullptr,
                                              c10::hip::getCurrentHIPStream(dev.index()).stream());
  check_rc(rc, "hgs_reduce_view_packs_unpack");
  return {m3, m2, sh, op, sc, ro, radii};
}

// ---- bookkeeping either side of the path (include/hgs_rast.h: hgs_densify_*, hgs_compact_*, hgs_reanchor)
void need_dev(const Tensor& t, const c10::Device& dev, at::ScalarType ty, const char* name) {
  if (t.device() != dev || t.scalar_type() != ty || !t.is_contiguous())
    throw std::runtime_error(std::string(name) + ": expected a contiguous tensor of the right dtype on " + dev.str());
}

// in-place update of xyz_gradient_accum / denom / max_radii2D; returns (radii_max int32 [P], visibility bool [P])
std::vector<Tensor> densify_stats(const Tensor& grad_means2D, const Tensor& radii, const c10::optional<Tensor>& keep,
                                  Tensor accum, Tensor denom, Tensor max_radii2D) {
  at::NoGradGuard ng;
  const c10::Device dev = radii.device();
  if (!dev.is_cuda()) throw std::runtime_error("humangaussian_amd: tensors must live on a HIP device");
  DeviceSwitch guard(dev.index());
  const Tensor r = radii.dim() == 1 ? radii.unsqueeze(0) : radii;
  const int64_t B = r.size(0), P = r.size(1);
  const Tensor g = f32c(grad_means2D, dev, "viewspace gradient");
  const Tensor rc = r.contiguous();
  if (rc.scalar_type() != at::kInt) throw std::runtime_error("radii must be int32");
  if (g.numel() != B * P * 3) throw std::runtime_error("viewspace gradient must have dimensions (views, num_points, 3)");
  need_dev(accum, dev, at::kFloat, "xyz_gradient_accum");
  need_dev(denom, dev, at::kFloat, "denom");
  need_dev(max_radii2D, dev, at::kFloat, "max_radii2D");
  if (accum.numel() != P || denom.numel() != P || max_radii2D.numel() != P)
    throw std::runtime_error("xyz_gradient_accum / denom / max_radii2D must have num_points elements");
  Tensor keep_u8;
  if (keep.has_value() && keep->defined()) {
    if (keep->device() != dev) throw std::runtime_error("keep mask must live on the device of radii");
    keep_u8 = keep->to(at::kByte).contiguous();
    if (keep_u8.numel() != P) throw std::runtime_error("keep mask must have num_points elements on the device");
  }
  Tensor rmax = at::empty({P}, rc.options());
  Tensor vis = at::empty({P}, rc.options().dtype(at::kByte));
  const int rcode = hgs_densify_stats((int32_t)B, (int32_t)P, fptr(g), P > 0 ? rc.data_ptr<int32_t>() : nullptr,
                                      keep_u8.defined() && P > 0 ? keep_u8.data_ptr<uint8_t>() : nullptr, fptr_mut(accum),
                                      fptr_mut(denom), fptr_mut(max_radii2D), P > 0 ? rmax.data_ptr<int32_t>() : nullptr,
                                      P > 0 ? vis.data_ptr<uint8_t>() : nullptr,
                                      c10::hip::getCurrentHIPStream(dev.index()).stream());
  check_rc(rcode, "hgs_densify_stats");
  return {rmax, vis.to(at::kBool)};
}

// returns (clone bool [P], split bool [P], prune bool [P], counts int32 [3] on the device)
std::vector<Tensor> densify_masks(const Tensor& accum, const Tensor& denom, const Tensor& scales, bool scales_are_log,
                                  const Tensor& opacity, bool opacity_is_logit, const Tensor& max_radii2D,
                                  double grad_threshold, double percent_dense, double extent, double min_opacity,
                                  double max_screen_size, double size_thresh) {
  at::NoGradGuard ng;
  const c10::Device dev = accum.device();
  if (!dev.is_cuda()) throw std::runtime_error("humangaussian_amd: tensors must live on a HIP device");
  DeviceSwitch guard(dev.index());
  const Tensor a = f32c(accum, dev, "xyz_gradient_accum"), d = f32c(denom, dev, "denom"), sc = f32c(scales, dev, "scales");
  const Tensor op = f32c(opacity, dev, "opacity"), mr = f32c(max_radii2D, dev, "max_radii2D");
  const int64_t P = a.numel();
  if (d.numel() != P || sc.numel() != 3 * P || op.numel() != P || mr.numel() != P)
    throw std::runtime_error("densify_masks: inconsistent shapes");
  const auto bopt = at::TensorOptions().dtype(at::kByte).device(dev);
  Tensor cl = at::empty({P}, bopt), sp = at::empty({P}, bopt), pr = at::empty({P}, bopt);
  Tensor counts = at::empty({3}, bopt.dtype(at::kInt));
  const int rc = hgs_densify_masks((int32_t)P, fptr(a), fptr(d), fptr(sc), scales_are_log ? 1 : 0, fptr(op),
                                   opacity_is_logit ? 1 : 0, fptr(mr), (float)grad_threshold, (float)percent_dense,
                                   (float)extent, (float)min_opacity, (float)max_screen_size, (float)size_thresh,
                                   P > 0 ? cl.data_ptr<uint8_t>() : nullptr, P > 0 ? sp.data_ptr<uint8_t>() : nullptr,
                                   P > 0 ? pr.data_ptr<uint8_t>() : nullptr,
                                   reinterpret_cast<uint32_t*>(counts.data_ptr<int32_t>()),
                                   c10::hip::getCurrentHIPStream(dev.index()).stream());
  check_rc(rc, "hgs_densify_masks");
  return {cl.to(at::kBool), sp.to(at::kBool), pr.to(at::kBool), counts};
}

// keeps the rows where keep[i] of every tensor in `tensors` (all [P, ...] fp32), order preserved: the
// pruning of all parameters and of both Adam moments with ONE index computation (one D2H read: the count)
std::vector<Tensor> compact_rows(const Tensor& keep, const std::vector<Tensor>& tensors) {
  at::NoGradGuard ng;
  const c10::Device dev = keep.device();
  if (!dev.is_cuda()) throw std::runtime_error("humangaussian_amd: tensors must live on a HIP device");
  DeviceSwitch guard(dev.index());
  for (const Tensor& t : tensors) {
    if (t.device() != dev) throw std::runtime_error("compact_rows: every tensor must live on the device of `keep`");
    if (t.scalar_type() != at::kFloat)
      throw std::runtime_error("compact_rows: fp32 tensors only (got " + std::string(c10::toString(t.scalar_type())) +
                               "): gather other dtypes with index_select on the returned row count");
    if (t.dim() < 1) throw std::runtime_error("compact_rows: tensors need a leading num_points dimension");
  }
  const Tensor k = keep.to(at::kByte).contiguous();
  const int64_t P = k.numel();
  hipStream_t stream = c10::hip::getCurrentHIPStream(dev.index()).stream();
  Tensor idx = at::empty({P}, at::TensorOptions().dtype(at::kInt).device(dev));
  Tensor cnt = at::empty({1}, at::TensorOptions().dtype(at::kInt).device(dev));
  Tensor scratch = at::empty({(int64_t)hgs_compact_scratch_bytes((int32_t)P)}, at::TensorOptions().dtype(at::kByte).device(dev));
  check_rc(hgs_compact_index((int32_t)P, P > 0 ? k.data_ptr<uint8_t>() : nullptr, P > 0 ? idx.data_ptr<int32_t>() : nullptr,
                             reinterpret_cast<uint32_t*>(cnt.data_ptr<int32_t>()), scratch.data_ptr(), stream),
           "hgs_compact_index");
  const int64_t n = cnt.item<int32_t>();
  std::vector<Tensor> out;
  for (const Tensor& t : tensors) {
    if (t.size(0) != P) throw std::runtime_error("compact_rows: every tensor needs num_points rows");
    const Tensor src = f32c(t, dev, "tensor");
    const int64_t rf = P > 0 ? src.numel() / P : 1;
    std::vector<int64_t> shape = src.sizes().vec();
    shape[0] = n;
    Tensor dst = at::empty(shape, src.options());
    check_rc(hgs_gather_rows(n, (int32_t)std::max<int64_t>(rf, 1), n > 0 ? idx.data_ptr<int32_t>() : nullptr, fptr(src),
                             fptr_mut(dst), stream), "hgs_gather_rows");
    out.push_back(dst);
  }
  return out;
}

Tensor reanchor(const Tensor& vertices, const Tensor& faces, const Tensor& mapping_face, const Tensor& mapping_uvw,
                const Tensor& mapping_dist) {
  at::NoGradGuard ng;
  const c10::Device dev = vertices.device();
  if (!dev.is_cuda()) throw std::runtime_error("humangaussian_amd: tensors must live on a HIP device");
  DeviceSwitch guard(dev.index());
  const Tensor v = f32c(vertices, dev, "vertices"), uvw = f32c(mapping_uvw, dev, "mapping_uvw"), dist = f32c(mapping_dist, dev, "mapping_dist");
  const Tensor f = faces.to(at::kInt).contiguous(), mf = mapping_face.to(at::kInt).contiguous();
  if (f.device() != dev || mf.device() != dev) throw std::runtime_error("faces / mapping_face must live on the same device");
  const int64_t P = mf.numel();
  if (uvw.numel() != 3 * P || dist.numel() != P || v.numel() % 3 || f.numel() % 3) throw std::runtime_error("reanchor: inconsistent shapes");
  Tensor xyz = at::empty({P, 3}, v.options());
  check_rc(hgs_reanchor((int32_t)P, fptr(v), f.numel() ? f.data_ptr<int32_t>() : nullptr, P > 0 ? mf.data_ptr<int32_t>() : nullptr,
                        fptr(uvw), fptr(dist), fptr_mut(xyz), c10::hip::getCurrentHIPStream(dev.index()).stream()),
           "hgs_reanchor");
  return xyz;
}

// hgs_reanchor_rot on the current stream, nothing read back -> (xyz [P,3], rot [P,4]).  bind: rot = conj(r) (x) rot_in at the
// rest mesh; else rot = r (x) rot_in at the posed mesh.  Both forms return the re-anchored positions.
std::vector<Tensor> reanchor_rot(const Tensor& vertices, const Tensor& faces, const Tensor& mapping_face,
                                 const Tensor& mapping_uvw, const Tensor& mapping_dist, const Tensor& rot_in, bool bind) {
  at::NoGradGuard ng;
  const c10::Device dev = vertices.device();
  if (!dev.is_cuda()) throw std::runtime_error("humangaussian_amd: tensors must live on a HIP device");
  DeviceSwitch guard(dev.index());
  const Tensor v = f32c(vertices, dev, "vertices"), uvw = f32c(mapping_uvw, dev, "mapping_uvw"), dist = f32c(mapping_dist, dev, "mapping_dist");
  const Tensor q = f32c(rot_in, dev, "rot_in");
  const Tensor f = faces.to(at::kInt).contiguous(), mf = mapping_face.to(at::kInt).contiguous();
  if (f.device() != dev || mf.device() != dev) throw std::runtime_error("faces / mapping_face must live on the same device");
  const int64_t P = mf.numel();
  if (uvw.numel() != 3 * P || dist.numel() != P || q.numel() != 4 * P || v.numel() % 3 || f.numel() % 3)
    throw std::runtime_error("reanchor_rot: inconsistent shapes");
  Tensor xyz = at::empty({P, 3}, v.options()), rot = at::empty({P, 4}, v.options());
  check_rc(hgs_reanchor_rot((int32_t)P, fptr(v), f.numel() ? f.data_ptr<int32_t>() : nullptr, P > 0 ? mf.data_ptr<int32_t>() : nullptr,
                            fptr(uvw), fptr(dist), fptr(q), bind ? 1 : 0, fptr_mut(xyz), fptr_mut(rot),
                            c10::hip::getCurrentHIPStream(dev.index()).stream()),
           "hgs_reanchor_rot");
  return {xyz, rot};
}

// ---- the optimizer step (include/hgs_rast.h: hgs_adam_step): every tensor of the lists in one launch per
// HGS_ADAM_MAX_TENSORS of them, on the current stream, nothing read back.  scalars[k] = the six floats of tensor k in the
// header's order (step_size, bc2_sqrt, w1, beta2, w2, eps), derived by the caller in double.  Nothing is converted or
// copied here: a tensor that is not fp32, contiguous and on the device of the first is an error (optim.py sends such
// parameters down torch's own path instead).
void adam_step(std::vector<Tensor> params, const std::vector<Tensor>& grads, std::vector<Tensor> exp_avgs,
               std::vector<Tensor> exp_avg_sqs, const std::vector<std::vector<double>>& scalars,
               const c10::optional<Tensor>& visible) {
  at::NoGradGuard ng;
  const size_t n = params.size();
  if (grads.size() != n || exp_avgs.size() != n || exp_avg_sqs.size() != n || scalars.size() != n)
    throw std::runtime_error("adam_step: params, grads, exp_avgs, exp_avg_sqs and scalars must have one entry per tensor");
  if (n == 0) return;
  const c10::Device dev = params[0].device();
  if (!dev.is_cuda()) throw std::runtime_error("humangaussian_amd: tensors must live on a HIP device");
  DeviceSwitch guard(dev.index());
  const uint8_t* vis = nullptr;
  int64_t vis_rows = 0;
  Tensor vis_u8;
  if (visible.has_value() && visible->defined()) {
    if (visible->device() != dev || !visible->is_contiguous() ||
        (visible->scalar_type() != at::kBool && visible->scalar_type() != at::kByte))
      throw std::runtime_error("adam_step: visible must be a contiguous bool or uint8 tensor on " + dev.str());
    vis_u8 = visible->scalar_type() == at::kBool ? visible->view(at::kByte) : *visible;      // (bool is one byte of 0 / 1)
    vis_rows = vis_u8.numel();
    if (vis_rows == 0) return;                       // no rows at all: nothing is visible
    vis = vis_u8.data_ptr<uint8_t>();
  }
  hipStream_t stream = c10::hip::getCurrentHIPStream(dev.index()).stream();
  for (size_t first = 0; first < n; first += HGS_ADAM_MAX_TENSORS) {
    hgs_adam_args a{};
    a.num_tensors = (int32_t)std::min<size_t>(HGS_ADAM_MAX_TENSORS, n - first);
    a.visible = vis;
    a.visible_rows = vis_rows;
    for (int32_t j = 0; j < a.num_tensors; ++j) {
      const size_t k = first + (size_t)j;
      need_dev(params[k], dev, at::kFloat, "adam_step: param");
      need_dev(grads[k], dev, at::kFloat, "adam_step: grad");
      need_dev(exp_avgs[k], dev, at::kFloat, "adam_step: exp_avg");
      need_dev(exp_avg_sqs[k], dev, at::kFloat, "adam_step: exp_avg_sq");
      const int64_t numel = params[k].numel();
      if (grads[k].numel() != numel || exp_avgs[k].numel() != numel || exp_avg_sqs[k].numel() != numel)
        throw std::runtime_error("adam_step: a tensor's grad, exp_avg and exp_avg_sq must have its number of elements");
      if (scalars[k].size() != 6) throw std::runtime_error("adam_step: six scalars per tensor");
      hgs_adam_tensor& t = a.t[j];
      t.rows = params[k].dim() >= 1 ? params[k].size(0) : 1;
      const int64_t rf = t.rows > 0 ? numel / t.rows : 0;
      if (rf > 0x7fffffffll) throw std::runtime_error("adam_step: rows of more than 2^31 - 1 elements are not supported");
      t.row_floats = (int32_t)rf;
      if (vis && t.rows != vis_rows)
        throw std::runtime_error("adam_step: visible has " + std::to_string(vis_rows) + " entries, a tensor has " +
                                 std::to_string(t.rows) + " rows");
      t.param = fptr_mut(params[k]);
      t.grad = fptr(grads[k]);
      t.exp_avg = fptr_mut(exp_avgs[k]);
      t.exp_avg_sq = fptr_mut(exp_avg_sqs[k]);
      t.step_size = (float)scalars[k][0];
      t.bc2_sqrt = (float)scalars[k][1];
      t.w1 = (float)scalars[k][2];
      t.beta2 = (float)scalars[k][3];
      t.w2 = (float)scalars[k][4];
      t.eps = (float)scalars[k][5];
    }
    check_rc(hgs_adam_step(&a, stream), "hgs_adam_step");
  }
}

// ---- posing a skinned body (include/hgs_rast.h: hgs_lbs_pose): F frames in two launches on the current stream, the
// workspace from the caching allocator, nothing read back.  Every tensor is what body.SkinnedBody keeps resident: fp32 /
// int32, contiguous, on one device - nothing is converted or copied here.  posedirs is the padded (K, stride) table or
// None (K = 0).  Returns (vertices (F, V, 3), joints (F, J, 3) or None).
std::tuple<Tensor, c10::optional<Tensor>> lbs_pose(const Tensor& v_shaped, const Tensor& J_rest, const Tensor& parents,
                                                   const c10::optional<Tensor>& posedirs, const Tensor& weight_joint,
                                                   const Tensor& weight_value, const Tensor& poses,
                                                   const c10::optional<Tensor>& transl, std::vector<double> centre, double scale,
                                                   bool return_joints) {
  at::NoGradGuard ng;
  const c10::Device dev = poses.device();
  if (!dev.is_cuda()) throw std::runtime_error("humangaussian_amd: tensors must live on a HIP device");
  DeviceSwitch guard(dev.index());
  need_dev(v_shaped, dev, at::kFloat, "lbs_pose: v_shaped");
  need_dev(J_rest, dev, at::kFloat, "lbs_pose: J_rest");
  need_dev(parents, dev, at::kInt, "lbs_pose: parents");
  need_dev(weight_joint, dev, at::kInt, "lbs_pose: weight_joint");
  need_dev(weight_value, dev, at::kFloat, "lbs_pose: weight_value");
  need_dev(poses, dev, at::kFloat, "lbs_pose: poses");
  if (poses.dim() != 3 || poses.size(2) != 3) throw std::runtime_error("lbs_pose: poses must be (F, J, 3)");
  const int64_t F = poses.size(0), J = poses.size(1), V = v_shaped.numel() / 3;
  if (J < 1 || J > HGS_LBS_MAX_JOINTS)
    throw std::runtime_error("lbs_pose: 1.." + std::to_string(HGS_LBS_MAX_JOINTS) + " joints, got " + std::to_string(J));
  if (v_shaped.numel() != 3 * V || J_rest.numel() != 3 * J || parents.numel() != J || V > (1 << 29) || F > 0x7fffffffll)
    throw std::runtime_error("lbs_pose: v_shaped (V, 3), J_rest (J, 3) and parents (J,) do not fit poses (F, J, 3)");
  if (weight_joint.dim() != 2 || weight_joint.size(0) != V || weight_value.sizes() != weight_joint.sizes())
    throw std::runtime_error("lbs_pose: weight_joint and weight_value must both be (V, width)");
  if (centre.size() != 3) throw std::runtime_error("lbs_pose: centre has three components");
  hgs_lbs_args a{};
  a.V = (int32_t)V; a.J = (int32_t)J; a.F = (int32_t)F;
  a.weight_width = (int32_t)std::min<int64_t>(weight_joint.size(1), 0x7fffffffll);
  if (posedirs.has_value() && posedirs->defined() && posedirs->numel() > 0) {
    need_dev(*posedirs, dev, at::kFloat, "lbs_pose: posedirs");
    if (posedirs->dim() != 2 || posedirs->size(0) != 9 * (J - 1) || posedirs->size(1) > 0x7fffffffll)
      throw std::runtime_error("lbs_pose: posedirs must be (9 (J - 1), stride)");
    a.K = (int32_t)posedirs->size(0);
    a.posedirs_stride = (int32_t)posedirs->size(1);
    a.posedirs = fptr(*posedirs);
  }
  if (transl.has_value() && transl->defined()) {
    need_dev(*transl, dev, at::kFloat, "lbs_pose: transl");
    if (transl->numel() != 3 * F) throw std::runtime_error("lbs_pose: transl must be (F, 3)");
    a.transl = fptr(*transl);
  }
  Tensor vertices = at::empty({F, V, 3}, poses.options());
  Tensor joints;
  if (return_joints) joints = at::empty({F, J, 3}, poses.options());
  Tensor work = at::empty({(int64_t)hgs_lbs_workspace_bytes((int32_t)J, (int32_t)F)}, at::TensorOptions().dtype(at::kByte).device(dev));
  a.v_shaped = fptr(v_shaped);
  a.J_rest = fptr(J_rest);
  a.parents = parents.data_ptr<int32_t>();
  a.weight_joint = V > 0 ? weight_joint.data_ptr<int32_t>() : nullptr;
  a.weight_value = fptr(weight_value);
  a.poses = fptr(poses);
  for (int c = 0; c < 3; ++c) a.centre[c] = (float)centre[c];
  a.scale = (float)scale;
  a.workspace = work.numel() ? work.data_ptr() : nullptr;
  a.vertices = fptr_mut(vertices);
  a.joints = return_joints ? fptr_mut(joints) : nullptr;
  check_rc(hgs_lbs_pose(&a, c10::hip::getCurrentHIPStream(dev.index()).stream()), "hgs_lbs_pose");
  if (return_joints && V == 0 && F > 0)
    throw std::runtime_error("lbs_pose: joints of a body without vertices are not computed");
  return {vertices, return_joints ? c10::optional<Tensor>(joints) : c10::nullopt};
}

// ---- pose-control images (include/hgs_rast.h: hgs_pose_draw): B views of one skeleton in one launch on the current
// stream, nothing read back.  points (K, 4) fp32, mvp (B, 4, 4) fp32, occlusion (B,) uint8 or None.  Returns (image
// (B, H, W, 3) fp32 or uint8, kp (B, K, 3), records (B, R, 8) int32).
std::tuple<Tensor, Tensor, Tensor> pose_draw(const Tensor& points, const Tensor& mvp, const c10::optional<Tensor>& occlusion,
                                             int64_t style, int64_t H, int64_t W, int64_t limb_width, bool uint8_out) {
  at::NoGradGuard ng;
  const c10::Device dev = mvp.device();
  if (!dev.is_cuda()) throw std::runtime_error("humangaussian_amd: tensors must live on a HIP device");
  DeviceSwitch guard(dev.index());
  need_dev(points, dev, at::kFloat, "pose_draw: points");
  need_dev(mvp, dev, at::kFloat, "pose_draw: mvp");
  if (style != HGS_POSE_OPENPOSE && style != HGS_POSE_HUMANSD) throw std::runtime_error("pose_draw: style is 0 (OpenPose) or 1 (HumanSD)");
  const int64_t K = style == HGS_POSE_HUMANSD ? 17 : 18;
  if (points.dim() != 2 || points.size(0) != K || points.size(1) != 4)
    throw std::runtime_error("pose_draw: points must be (" + std::to_string(K) + ", 4) for this style");
  if (mvp.dim() != 3 || mvp.size(1) != 4 || mvp.size(2) != 4) throw std::runtime_error("pose_draw: mvp must be (B, 4, 4)");
  const int64_t B = mvp.size(0);
  if (B > 65535) throw std::runtime_error("pose_draw: at most 65535 views");
  if (H < 1 || H > HGS_POSE_MAX_DIM || W < 1 || W > HGS_POSE_MAX_DIM)
    throw std::runtime_error("pose_draw: H and W must be in [1, " + std::to_string(HGS_POSE_MAX_DIM) + "]");
  if (limb_width < 1 || limb_width > 32767) throw std::runtime_error("pose_draw: limb_width must be in [1, 32767], got " + std::to_string(limb_width));
  hgs_pose_args a{};
  a.style = (int32_t)style; a.B = (int32_t)B; a.K = (int32_t)K; a.H = (int32_t)H; a.W = (int32_t)W;
  a.limb_width = (int32_t)limb_width;
  a.uint8_out = uint8_out ? 1 : 0;
  if (occlusion.has_value() && occlusion->defined()) {
    need_dev(*occlusion, dev, at::kByte, "pose_draw: occlusion");
    if (occlusion->numel() != B) throw std::runtime_error("pose_draw: occlusion must be (B,)");
    a.occlusion = B > 0 ? occlusion->data_ptr<uint8_t>() : nullptr;
  }
  const int64_t R = (int64_t)(hgs_pose_records_bytes(a.style, 1) / (HGS_POSE_RECORD_INTS * sizeof(int32_t)));
  Tensor image = at::empty({B, H, W, 3}, mvp.options().dtype(uint8_out ? at::kByte : at::kFloat));
  Tensor kp = at::empty({B, K, 3}, mvp.options());
  Tensor records = at::empty({B, R, HGS_POSE_RECORD_INTS}, mvp.options().dtype(at::kInt));
  a.points = fptr(points);
  a.mvp = fptr(mvp);
  a.image = B > 0 ? image.data_ptr() : nullptr;
  a.kp = fptr_mut(kp);
  a.records = B > 0 ? records.data_ptr<int32_t>() : nullptr;
  check_rc(hgs_pose_draw(&a, c10::hip::getCurrentHIPStream(dev.index()).stream()), "hgs_pose_draw");
  return {image, kp, records};
}

// ---- the step's guidance images and opacity losses (include/hgs_rast.h: hgs_step_images_*): three launches each way on
// the current stream, the workspace from the caching allocator, nothing read back.  render (B, 3, H, W) and depth
// (B, 1, H, W) fp32 contiguous.  Forward returns (rgb, depth3 (B, 3, h, w) fp32 or fp16, loss_sparsity, loss_opaque (0-dim),
// depth_min, depth_max (B,), depth_global_max (0-dim), tie_counts (2 B + 1,) int32).
namespace {
const void* si_aligned(Tensor& t) {   // the kernels take 16-byte accesses: a view into the middle of a storage is copied
  if (((uintptr_t)t.data_ptr() & 15) != 0) t = t.clone();
  return t.data_ptr();
}
hgs_step_images_args si_args(const Tensor& depth, int64_t h, int64_t w, bool half_images, const char* who) {
  if (depth.dim() != 4 || depth.size(1) != 1) throw std::runtime_error(std::string(who) + ": depth must be (B, 1, H, W)");
  const int64_t B = depth.size(0), H = depth.size(2), W = depth.size(3);
  if (B < 1 || B > 65535 || H < 1 || W < 1 || H > HGS_SI_MAX_DIM || W > HGS_SI_MAX_DIM || B * H * W > 0x7fffffffll)
    throw std::runtime_error(std::string(who) + ": 1..65535 views of at most " + std::to_string(HGS_SI_MAX_DIM) + " pixels a side, fewer than 2^31 pixels in all");
  if (h < 1 || w < 1 || h > H || w > W) throw std::runtime_error(std::string(who) + ": the output size must be within [1, H] x [1, W] (no upsampling)");
  hgs_step_images_args a{};
  a.B = (int32_t)B; a.H = (int32_t)H; a.W = (int32_t)W; a.h = (int32_t)h; a.w = (int32_t)w;
  a.half_images = half_images ? 1 : 0;
  return a;
}
Tensor si_workspace(const hgs_step_images_args& a, const c10::Device& dev) {
  return at::empty({(int64_t)hgs_step_images_workspace_bytes(a.B, a.H, a.W, a.h, a.w)}, at::TensorOptions().dtype(at::kByte).device(dev));
}
}  // namespace

std::vector<Tensor> step_images_forward(Tensor render, Tensor depth, int64_t h, int64_t w, bool half_images) {
  at::NoGradGuard ng;
  const c10::Device dev = depth.device();
  if (!dev.is_cuda()) throw std::runtime_error("humangaussian_amd: tensors must live on a HIP device");
  DeviceSwitch guard(dev.index());
  need_dev(render, dev, at::kFloat, "step_images_forward: render");
  need_dev(depth, dev, at::kFloat, "step_images_forward: depth");
  hgs_step_images_args a = si_args(depth, h, w, half_images, "step_images_forward");
  if (render.dim() != 4 || render.size(0) != a.B || render.size(1) != 3 || render.size(2) != a.H || render.size(3) != a.W)
    throw std::runtime_error("step_images_forward: render must be (B, 3, H, W) with depth's B, H, W");
  const auto fopt = depth.options();
  const auto iopt = fopt.dtype(half_images ? at::kHalf : at::kFloat);
  Tensor rgb = at::empty({a.B, 3, h, w}, iopt), depth3 = at::empty({a.B, 3, h, w}, iopt);
  Tensor ls = at::empty({}, fopt), lo = at::empty({}, fopt), gmax = at::empty({}, fopt), dmin = at::empty({a.B}, fopt), dmax = at::empty({a.B}, fopt);
  Tensor counts = at::empty({2 * (int64_t)a.B + 1}, fopt.dtype(at::kInt));
  Tensor work = si_workspace(a, dev);
  a.render = static_cast<const float*>(si_aligned(render));
  a.depth = static_cast<const float*>(si_aligned(depth));
  a.workspace = work.data_ptr();
  a.rgb_out = rgb.data_ptr();
  a.depth_out = depth3.data_ptr();
  a.loss_sparsity = ls.data_ptr<float>();
  a.loss_opaque = lo.data_ptr<float>();
  a.depth_global_max = gmax.data_ptr<float>();
  a.depth_min = dmin.data_ptr<float>();
  a.depth_max = dmax.data_ptr<float>();
  a.tie_counts = reinterpret_cast<uint32_t*>(counts.data_ptr<int32_t>());
  check_rc(hgs_step_images_forward(&a, c10::hip::getCurrentHIPStream(dev.index()).stream()), "hgs_step_images_forward");
  return {rgb, depth3, ls, lo, dmin, dmax, gmax, counts};
}

// The gradient of the above.  depth and the forward's depth_min / depth_max / depth_global_max / tie_counts; the four
// incoming gradients, each optional (None: absent).  Returns (grad_render or None, grad_depth or None).
std::tuple<c10::optional<Tensor>, c10::optional<Tensor>> step_images_backward(
    Tensor depth, const Tensor& dmin, const Tensor& dmax, const Tensor& gmax, const Tensor& counts, int64_t h, int64_t w,
    bool half_images, c10::optional<Tensor> grad_rgb, c10::optional<Tensor> grad_depth, c10::optional<Tensor> grad_ls,
    c10::optional<Tensor> grad_lo) {
  at::NoGradGuard ng;
  const c10::Device dev = depth.device();
  if (!dev.is_cuda()) throw std::runtime_error("humangaussian_amd: tensors must live on a HIP device");
  DeviceSwitch guard(dev.index());
  need_dev(depth, dev, at::kFloat, "step_images_backward: depth");
  need_dev(dmin, dev, at::kFloat, "step_images_backward: depth_min");
  need_dev(dmax, dev, at::kFloat, "step_images_backward: depth_max");
  need_dev(gmax, dev, at::kFloat, "step_images_backward: depth_global_max");
  need_dev(counts, dev, at::kInt, "step_images_backward: tie_counts");
  hgs_step_images_args a = si_args(depth, h, w, half_images, "step_images_backward");
  if (dmin.numel() != a.B || dmax.numel() != a.B || gmax.numel() != 1 || counts.numel() != 2 * (int64_t)a.B + 1)
    throw std::runtime_error("step_images_backward: depth_min / depth_max (B,), depth_global_max (1), tie_counts (2 B + 1,)");
  const at::ScalarType ity = half_images ? at::kHalf : at::kFloat;
  auto image_grad = [&](c10::optional<Tensor>& g, const char* name) -> const void* {
    if (!g.has_value() || !g->defined()) return nullptr;
    need_dev(*g, dev, ity, name);
    if (g->numel() != (int64_t)a.B * 3 * h * w) throw std::runtime_error(std::string(name) + " must be (B, 3, h, w)");
    return si_aligned(*g);
  };
  auto scalar_grad = [&](c10::optional<Tensor>& g, const char* name) -> const float* {
    if (!g.has_value() || !g->defined()) return nullptr;
    need_dev(*g, dev, at::kFloat, name);
    if (g->numel() != 1) throw std::runtime_error(std::string(name) + " must have one element");
    return g->data_ptr<float>();
  };
  a.grad_rgb = image_grad(grad_rgb, "step_images_backward: grad_rgb");
  a.grad_depth = image_grad(grad_depth, "step_images_backward: grad_depth");
  a.grad_loss_sparsity = scalar_grad(grad_ls, "step_images_backward: grad_loss_sparsity");
  a.grad_loss_opaque = scalar_grad(grad_lo, "step_images_backward: grad_loss_opaque");
  const bool want_depth = a.grad_depth || a.grad_loss_sparsity || a.grad_loss_opaque;
  Tensor d_render, d_depth, work;
  if (a.grad_rgb) d_render = at::empty({a.B, 3, a.H, a.W}, depth.options());
  if (want_depth) {
    d_depth = at::empty({a.B, 1, a.H, a.W}, depth.options());
    work = si_workspace(a, dev);
    a.workspace = work.data_ptr();
  }
  a.depth = static_cast<const float*>(si_aligned(depth));
  a.depth_min = const_cast<float*>(dmin.data_ptr<float>());
  a.depth_max = const_cast<float*>(dmax.data_ptr<float>());
  a.depth_global_max = const_cast<float*>(gmax.data_ptr<float>());
  a.tie_counts = reinterpret_cast<uint32_t*>(const_cast<int32_t*>(counts.data_ptr<int32_t>()));
  a.grad_render = a.grad_rgb ? d_render.data_ptr<float>() : nullptr;
  a.grad_depth_in = want_depth ? d_depth.data_ptr<float>() : nullptr;
  check_rc(hgs_step_images_backward(&a, c10::hip::getCurrentHIPStream(dev.index()).stream()), "hgs_step_images_backward");
  return {a.grad_rgb ? c10::optional<Tensor>(d_render) : c10::nullopt, want_depth ? c10::optional<Tensor>(d_depth) : c10::nullopt};
}

// ---- the photometric loss (include/hgs_rast.h: hgs_photometric_*): two launches forward and one backward on the current
// stream, the workspace from the caching allocator, nothing read back.  image and gt (B, C, H, W) fp32 contiguous.  Forward
// returns (loss, l1, ssim (0-dim), ssim_image (B,), sqerr (B, C), psnr (B,) or (B C,), workspace); with_grad = false leaves
// the derivative maps out of the workspace, which then cannot be handed to the backward.
namespace {
hgs_photometric_args pm_args(const Tensor& image, const Tensor& gt, double weight_l1, double weight_dssim, const char* who) {
  if (image.dim() != 4 || gt.sizes() != image.sizes()) throw std::runtime_error(std::string(who) + ": image and gt must be (B, C, H, W) of one shape");
  const int64_t B = image.size(0), C = image.size(1), H = image.size(2), W = image.size(3);
  if (B < 1 || C < 1 || H < 1 || W < 1 || H > HGS_SI_MAX_DIM || W > HGS_SI_MAX_DIM || B * C > 65535 || B * C * H * W > 0x7fffffffll)
    throw std::runtime_error(std::string(who) + ": 1..65535 planes of 1.." + std::to_string(HGS_SI_MAX_DIM) + " pixels a side, fewer than 2^31 elements in all");
  hgs_photometric_args a{};
  a.B = (int32_t)B; a.C = (int32_t)C; a.H = (int32_t)H; a.W = (int32_t)W;
  a.weight_l1 = (float)weight_l1;
  a.weight_dssim = (float)weight_dssim;
  a.image = image.data_ptr<float>();
  a.gt = gt.data_ptr<float>();
  return a;
}
}  // namespace

std::vector<Tensor> photometric_forward(const Tensor& image, const Tensor& gt, double weight_l1, double weight_dssim,
                                        bool psnr_per_plane, bool with_grad) {
  at::NoGradGuard ng;
  const c10::Device dev = image.device();
  if (!dev.is_cuda()) throw std::runtime_error("humangaussian_amd: tensors must live on a HIP device");
  DeviceSwitch guard(dev.index());
  need_dev(image, dev, at::kFloat, "photometric_forward: image");
  need_dev(gt, dev, at::kFloat, "photometric_forward: gt");
  hgs_photometric_args a = pm_args(image, gt, weight_l1, weight_dssim, "photometric_forward");
  a.with_grad = with_grad ? 1 : 0;
  a.psnr_per_plane = psnr_per_plane ? 1 : 0;
  const auto fopt = image.options();
  Tensor loss = at::empty({}, fopt), l1 = at::empty({}, fopt), ssim = at::empty({}, fopt), ssim_image = at::empty({a.B}, fopt);
  Tensor sqerr = at::empty({a.B, a.C}, fopt), psnr = at::empty({psnr_per_plane ? (int64_t)a.B * a.C : (int64_t)a.B}, fopt);
  Tensor work = at::empty({(int64_t)hgs_photometric_workspace_bytes(a.B, a.C, a.H, a.W, a.with_grad)}, fopt.dtype(at::kByte));
  a.workspace = work.data_ptr();
  a.loss = loss.data_ptr<float>();
  a.l1 = l1.data_ptr<float>();
  a.ssim = ssim.data_ptr<float>();
  a.ssim_image = ssim_image.data_ptr<float>();
  a.sqerr = sqerr.data_ptr<float>();
  a.psnr = psnr.data_ptr<float>();
  check_rc(hgs_photometric_forward(&a, c10::hip::getCurrentHIPStream(dev.index()).stream()), "hgs_photometric_forward");
  return {loss, l1, ssim, ssim_image, sqerr, psnr, work};
}

// The gradient with respect to image.  The forward's workspace (with_grad = true); the four incoming gradients, each
// optional (None: absent).  Returns None when all four are absent.
c10::optional<Tensor> photometric_backward(const Tensor& image, const Tensor& gt, const Tensor& workspace, double weight_l1,
                                           double weight_dssim, c10::optional<Tensor> grad_loss, c10::optional<Tensor> grad_l1,
                                           c10::optional<Tensor> grad_ssim, c10::optional<Tensor> grad_ssim_image) {
  at::NoGradGuard ng;
  const c10::Device dev = image.device();
  if (!dev.is_cuda()) throw std::runtime_error("humangaussian_amd: tensors must live on a HIP device");
  DeviceSwitch guard(dev.index());
  need_dev(image, dev, at::kFloat, "photometric_backward: image");
  need_dev(gt, dev, at::kFloat, "photometric_backward: gt");
  need_dev(workspace, dev, at::kByte, "photometric_backward: workspace");
  hgs_photometric_args a = pm_args(image, gt, weight_l1, weight_dssim, "photometric_backward");
  if (workspace.numel() != (int64_t)hgs_photometric_workspace_bytes(a.B, a.C, a.H, a.W, 1))
    throw std::runtime_error("photometric_backward: the workspace must be that of a forward with with_grad = true");
  auto grad = [&](c10::optional<Tensor>& g, int64_t n, const char* name) -> const float* {
    if (!g.has_value() || !g->defined()) return nullptr;
    need_dev(*g, dev, at::kFloat, name);
    if (g->numel() != n) throw std::runtime_error(std::string(name) + " has " + std::to_string(g->numel()) + " elements, expected " + std::to_string(n));
    return g->data_ptr<float>();
  };
  a.grad_loss = grad(grad_loss, 1, "photometric_backward: grad_loss");
  a.grad_l1 = grad(grad_l1, 1, "photometric_backward: grad_l1");
  a.grad_ssim = grad(grad_ssim, 1, "photometric_backward: grad_ssim");
  a.grad_ssim_image = grad(grad_ssim_image, a.B, "photometric_backward: grad_ssim_image");
  if (!a.grad_loss && !a.grad_l1 && !a.grad_ssim && !a.grad_ssim_image) return c10::nullopt;
  Tensor d_image = at::empty_like(image);
  a.workspace = workspace.data_ptr();
  a.grad_image = d_image.data_ptr<float>();
  check_rc(hgs_photometric_backward(&a, c10::hip::getCurrentHIPStream(dev.index()).stream()), "hgs_photometric_backward");
  return d_image;
}

void set_stage_events(const c10::optional<std::vector<int64_t>>& fwd, const c10::optional<std::vector<int64_t>>& bwd) {
  g_stage_fwd.clear();
  g_stage_bwd.clear();
  if (fwd) for (int64_t hnd : *fwd) g_stage_fwd.push_back(reinterpret_cast<void*>(hnd));
  if (bwd) for (int64_t hnd : *bwd) g_stage_bwd.push_back(reinterpret_cast<void*>(hnd));
  if (!g_stage_fwd.empty() && g_stage_fwd.size() != HGS_FWD_STAGES) throw std::runtime_error("fwd needs HGS_FWD_STAGES events");
  if (!g_stage_bwd.empty() && g_stage_bwd.size() != HGS_BWD_STAGES) throw std::runtime_error("bwd needs HGS_BWD_STAGES events");
}

py::dict device_state(int64_t dev) {
  {
    std::lock_guard<std::mutex> lk(g_mu);
    if (dev < 0 || dev >= (int64_t)g_states.size()) throw std::runtime_error("bad device index");
    if (!g_states[dev]) return py::dict();             // nothing has run on this device yet: no state is created here
  }
  DevState& st = state_for((int)dev);
  std::lock_guard<std::mutex> lk(st.mu);
  py::dict d;
  d["capacity"] = st.last_capacity;
  d["tile_hint"] = st.last_hint;
  d["max_R"] = st.max_R;
  d["max_tile"] = st.max_tile;
  d["calls"] = st.calls;
  d["retries"] = st.retries;
  d["wait_ns"] = st.wait_ns;
  d["bwd_pairs_last"] = st.last_pairs;          // pair count the last backward sized its scratch by (0: worst case)
  d["bwd_scratch_last"] = st.last_scratch;
  {
    static const char* names[8] = {"fwd_pre", "fwd_launch", "fwd_shadow", "fwd_wait", "fwd_total", "bwd_pre", "bwd_launch", "bwd_total"};
    py::dict hn;
    for (int i = 0; i < 8; ++i) hn[names[i]] = st.host_ns[i].load();
    d["host_ns"] = hn;
  }
  py::dict e;
  for (const auto& kv : st.est)
    e[py::make_tuple(std::get<0>(kv.first), std::get<1>(kv.first), std::get<2>(kv.first))] =
        py::make_tuple(kv.second.capacity, kv.second.tile_hint);
  d["estimates"] = e;
  return d;
}

}  // namespace

// ---- closest point / signed distance to a triangle mesh (include/hgs_rast.h: hgs_mesh_*; the reference's cubvh) -----
namespace {
std::pair<Tensor, Tensor> mesh_inputs(const Tensor& vertices, const Tensor& faces, const c10::Device& dev) {
  if (vertices.dim() != 2 || vertices.size(1) != 3) throw std::runtime_error("vertices must have dimensions (V, 3)");
  if (faces.dim() != 2 || faces.size(1) != 3) throw std::runtime_error("faces must have dimensions (F, 3)");
  if (faces.device() != dev) throw std::runtime_error("expected faces on " + dev.str() + ", got " + faces.device().str());
  if (at::isFloatingType(faces.scalar_type())) throw std::runtime_error("faces must hold integer vertex indices");
  if (vertices.size(0) > 0x7fffffffll / 3 || faces.size(0) > 0x7fffffffll / 48)
    throw std::runtime_error("mesh too large");
  return {f32c(vertices, dev, "vertices"), faces.to(at::kInt).contiguous()};
}
}  // namespace

// Plan + build of the uniform grid: one host wait (the plan's header decides the grid's size).  Returns (grid bytes,
// [dims x, y, z, ncells, num_refs]).  F == 0: an empty grid (queries of P > 0 points then fail).
std::tuple<Tensor, std::vector<int64_t>> mesh_build(const Tensor& vertices, const Tensor& faces) {
  at::NoGradGuard ng;
  const c10::Device dev = vertices.device();
  if (!dev.is_cuda()) throw std::runtime_error("humangaussian_amd: tensors must live on a HIP device");
  DeviceSwitch guard(dev.index());
  const auto vf = mesh_inputs(vertices, faces, dev);
  const Tensor &v = vf.first, &f = vf.second;
  const int64_t V = v.size(0), F = f.size(0);
  const auto byte_opts = at::TensorOptions().dtype(at::kByte).device(dev);
  if (F == 0) return {at::empty({0}, byte_opts), {0, 0, 0, 0, 0}};
  const int64_t lo = f.min().item<int64_t>(), hi = f.max().item<int64_t>();
  if (lo < 0 || hi >= V)
    throw std::runtime_error("faces index vertices outside [0, " + std::to_string(V) + "): min " + std::to_string(lo) +
                             ", max " + std::to_string(hi));
  hipStream_t stream = c10::hip::getCurrentHIPStream(dev.index()).stream();
  Tensor info_dev = at::empty({(int64_t)sizeof(hgs_mesh_grid_info)}, byte_opts);
  auto* info_ptr = reinterpret_cast<hgs_mesh_grid_info*>(info_dev.data_ptr());
  check_rc(hgs_mesh_grid_plan((int32_t)V, fptr(v), (int32_t)F, f.data_ptr<int32_t>(), info_ptr, stream), "hgs_mesh_grid_plan");
  hgs_mesh_grid_info info;
  if (hipMemcpyAsync(&info, info_ptr, sizeof(info), hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess)
    throw std::runtime_error("mesh_build: reading the grid plan failed");
  const size_t bytes = hgs_mesh_grid_bytes(&info);
  if (bytes == 0)
    throw std::runtime_error("mesh_build: the grid plan is unusable (" + std::to_string(info.num_refs) +
                             " face references; at most 2^31 - 1)");
  Tensor grid = at::empty({(int64_t)bytes}, byte_opts);
  check_rc(hgs_mesh_grid_build((int32_t)V, fptr(v), (int32_t)F, f.data_ptr<int32_t>(), &info, grid.data_ptr(), stream),
           "hgs_mesh_grid_build");
  return {grid, {info.dims[0], info.dims[1], info.dims[2], (int64_t)info.ncells, (int64_t)info.num_refs}};
}

// (dist [P] fp32, face [P] int32, uvw [P, 3] fp32 or undefined).  grid: mesh_build's, or None = brute force.
std::tuple<Tensor, Tensor, c10::optional<Tensor>> mesh_query(const Tensor& points, const Tensor& vertices,
                                                             const Tensor& faces, const c10::optional<Tensor>& grid,
                                                             bool raystab, bool want_uvw) {
  at::NoGradGuard ng;
  const c10::Device dev = points.device();
  if (!dev.is_cuda()) throw std::runtime_error("humangaussian_amd: tensors must live on a HIP device");
  if (points.dim() != 2 || points.size(1) != 3) throw std::runtime_error("points must have dimensions (P, 3)");
  if (points.size(0) > 0x7fffffffll / 3) throw std::runtime_error("too many points");
  DeviceSwitch guard(dev.index());
  const auto vf = mesh_inputs(vertices, faces, dev);
  const Tensor &v = vf.first, &f = vf.second;
  const Tensor pts = f32c(points, dev, "points");
  const bool use_grid = grid.has_value() && grid->defined() && grid->numel() > 0;
  if (use_grid && (grid->device() != dev || grid->scalar_type() != at::kByte))
    throw std::runtime_error("grid must be the uint8 tensor mesh_build returned, on the points' device");
  const int64_t P = pts.size(0);
  const auto opts = at::TensorOptions().device(dev);
  Tensor dist = at::empty({P}, opts.dtype(at::kFloat)), face = at::empty({P}, opts.dtype(at::kInt));
  c10::optional<Tensor> uvw;
  if (want_uvw) uvw = at::empty({P, 3}, opts.dtype(at::kFloat));
  if (P > 0 && f.size(0) == 0) throw std::runtime_error("mesh query: the mesh has no faces");
  check_rc(hgs_mesh_query((int32_t)P, fptr(pts), (int32_t)v.size(0), fptr(v), (int32_t)f.size(0),
                          f.numel() ? f.data_ptr<int32_t>() : nullptr, use_grid ? grid->data_ptr() : nullptr,
                          raystab ? HGS_MESH_RAYSTAB : HGS_MESH_UNSIGNED, dist.data_ptr<float>(), face.data_ptr<int32_t>(),
                          want_uvw && P > 0 ? uvw->data_ptr<float>() : nullptr,
                          c10::hip::getCurrentHIPStream(dev.index()).stream()),
           "hgs_mesh_query");
  return {dist, face, uvw};
}

// ---- density field and marching cubes (include/hgs_rast.h: hgs_field_*, hgs_mc_*; the reference's extract_fields / mcubes) ----
// (occ [R, R, R] fp32, block counts [nb, nb, nb] int32 or undefined, [center x, y, z, extent, scale], [num_kept, num_refs]).
// One host wait (the plan's header sizes the lists).  Nothing kept: a zero field and no evaluation.
// (`plan`, `lists` and `info` are what hgs_fsample needs to evaluate the same field at other points; lists stays undefined
// where nothing is listed.)
struct FieldBuilt {
  Tensor occ;
  c10::optional<Tensor> counts;
  std::vector<double> geo;
  std::vector<int64_t> sizes;
  Tensor plan, lists;
  hgs_field_info info;
};
FieldBuilt field_build_impl(
    const Tensor& xyz, const Tensor& opacity, const Tensor& scaling, const Tensor& rotation, const Tensor& axis,
    int64_t num_blocks, double grow, bool want_counts) {
  at::NoGradGuard ng;
  const c10::Device dev = xyz.device();
  if (!dev.is_cuda()) throw std::runtime_error("humangaussian_amd: tensors must live on a HIP device");
  if (xyz.dim() != 2 || xyz.size(1) != 3) throw std::runtime_error("xyz must have dimensions (P, 3)");
  const int64_t P = xyz.size(0), R = axis.numel();
  if (P > 0x7fffffffll / 16) throw std::runtime_error("too many Gaussians");
  if (opacity.numel() != P || scaling.numel() != 3 * P || rotation.numel() != 4 * P)
    throw std::runtime_error("opacity (P[, 1]), scaling (P, 3) and rotation (P, 4) must match xyz (P, 3)");
  if (axis.dim() != 1) throw std::runtime_error("axis must have dimensions (resolution,)");
  if (num_blocks < 1 || num_blocks > 32 || R < num_blocks || R > 2048 || R % num_blocks != 0 || R / num_blocks > 256)
    throw std::runtime_error("field: need 1 <= num_blocks <= 32, resolution <= 2048, resolution % num_blocks == 0 and "
                             "resolution / num_blocks <= 256");
  DeviceSwitch guard(dev.index());
  const Tensor x = f32c(xyz, dev, "xyz"), o = f32c(opacity, dev, "opacity"), s = f32c(scaling, dev, "scaling"),
               q = f32c(rotation, dev, "rotation"), ax = f32c(axis, dev, "axis");
  const auto opts = at::TensorOptions().device(dev);
  hipStream_t stream = c10::hip::getCurrentHIPStream(dev.index()).stream();
  const int32_t nb = (int32_t)num_blocks;
  Tensor plan = at::empty({(int64_t)hgs_field_plan_bytes((int32_t)P, nb)}, opts.dtype(at::kByte));
  Tensor info_dev = at::empty({(int64_t)sizeof(hgs_field_info)}, opts.dtype(at::kByte));
  auto* info_ptr = reinterpret_cast<hgs_field_info*>(info_dev.data_ptr());
  check_rc(hgs_field_plan((int32_t)P, fptr(x), fptr(o), fptr(s), fptr(q), (int32_t)R, nb, fptr(ax), (float)grow,
                          plan.data_ptr(), info_ptr, stream), "hgs_field_plan");
  hgs_field_info info;
  if (hipMemcpyAsync(&info, info_ptr, sizeof(info), hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess)
    throw std::runtime_error("field_extract: reading the plan failed");
  c10::optional<Tensor> counts;
  const std::vector<double> geo = {info.center[0], info.center[1], info.center[2], info.extent, info.scale};
  const std::vector<int64_t> sizes = {(int64_t)info.num_kept, (int64_t)info.num_refs};
  if (info.num_refs == 0) {
    if (want_counts) counts = at::zeros({num_blocks, num_blocks, num_blocks}, opts.dtype(at::kInt));
    return {at::zeros({R, R, R}, opts.dtype(at::kFloat)), counts, geo, sizes, plan, Tensor(), info};
  }
  const size_t bytes = hgs_field_list_bytes(&info);
  if (bytes == 0)
    throw std::runtime_error("field_extract: the plan is unusable (" + std::to_string(info.num_refs) +
                             " list entries; at most 2^31 - 1)");
  Tensor lists = at::empty({(int64_t)bytes}, opts.dtype(at::kByte));
  Tensor occ = at::empty({R, R, R}, opts.dtype(at::kFloat));
  if (want_counts) counts = at::empty({num_blocks, num_blocks, num_blocks}, opts.dtype(at::kInt));
  check_rc(hgs_field_eval(&info, fptr(ax), plan.data_ptr(), lists.data_ptr(), occ.data_ptr<float>(),
                          want_counts ? counts->data_ptr<int32_t>() : nullptr, stream), "hgs_field_eval");
  return {occ, counts, geo, sizes, plan, lists, info};
}

std::tuple<Tensor, c10::optional<Tensor>, std::vector<double>, std::vector<int64_t>> field_extract(
    const Tensor& xyz, const Tensor& opacity, const Tensor& scaling, const Tensor& rotation, const Tensor& axis,
    int64_t num_blocks, double grow, bool want_counts) {
  FieldBuilt b = field_build_impl(xyz, opacity, scaling, rotation, axis, num_blocks, grow, want_counts);
  return {b.occ, b.counts, b.geo, b.sizes};
}

// field_extract's results, then what a later field_sample needs: plan, lists (no element where nothing is listed) and the
// plan's header as 72 bytes on the host
std::tuple<Tensor, c10::optional<Tensor>, std::vector<double>, std::vector<int64_t>, Tensor, Tensor, Tensor> field_build(
    const Tensor& xyz, const Tensor& opacity, const Tensor& scaling, const Tensor& rotation, const Tensor& axis,
    int64_t num_blocks, double grow, bool want_counts) {
  FieldBuilt b = field_build_impl(xyz, opacity, scaling, rotation, axis, num_blocks, grow, want_counts);
  Tensor info = at::empty({(int64_t)sizeof(hgs_field_info)}, at::TensorOptions().dtype(at::kByte));
  memcpy(info.data_ptr(), &b.info, sizeof(hgs_field_info));
  if (!b.lists.defined()) b.lists = at::empty({0}, at::TensorOptions().device(xyz.device()).dtype(at::kByte));
  return {b.occ, b.counts, b.geo, b.sizes, b.plan, b.lists, info};
}

// (density [M], normal [M, 3], color [M, 3] or undefined) of the field at `points`; no host wait
std::tuple<Tensor, Tensor, c10::optional<Tensor>> field_sample(
    const Tensor& info, const Tensor& axis, const Tensor& plan, const Tensor& lists, const Tensor& points,
    const c10::optional<Tensor>& colors, bool normalized) {
  at::NoGradGuard ng;
  const c10::Device dev = points.device();
  if (!dev.is_cuda()) throw std::runtime_error("humangaussian_amd: tensors must live on a HIP device");
  if (points.dim() != 2 || points.size(1) != 3) throw std::runtime_error("points must have dimensions (M, 3)");
  if (info.device().is_cuda() || info.scalar_type() != at::kByte || !info.is_contiguous() ||
      info.numel() != (int64_t)sizeof(hgs_field_info))
    throw std::runtime_error("field_sample: info is the header field_build returned");
  hgs_field_info in;
  memcpy(&in, info.data_ptr(), sizeof(in));
  const int64_t M = points.size(0);
  if (M > 0x7fffffffll / 16) throw std::runtime_error("too many points");
  if (axis.dim() != 1 || axis.numel() != in.resolution) throw std::runtime_error("axis must have dimensions (resolution,)");
  if (plan.device() != dev || lists.device() != dev || axis.device() != dev)
    throw std::runtime_error("field_sample: the field and the points live on different devices");
  if ((size_t)plan.numel() != hgs_field_plan_bytes(in.num_gaussians, in.num_blocks))
    throw std::runtime_error("field_sample: plan does not belong to info");
  if (in.num_refs > 0 && (size_t)lists.numel() != hgs_field_list_bytes(&in))
    throw std::runtime_error("field_sample: lists do not belong to info");
  if (colors && (colors->dim() != 2 || colors->size(0) != in.num_gaussians || colors->size(1) != 3))
    throw std::runtime_error("colors must have dimensions (P, 3)");
  DeviceSwitch guard(dev.index());
  const auto opts = at::TensorOptions().device(dev).dtype(at::kFloat);
  const Tensor pts = f32c(points, dev, "points"), ax = f32c(axis, dev, "axis");
  Tensor col;
  if (colors) col = f32c(*colors, dev, "colors");
  Tensor density = at::empty({M}, opts), normal = at::empty({M, 3}, opts);
  c10::optional<Tensor> color;
  if (colors) color = at::empty({M, 3}, opts);
  if (M == 0) return {density, normal, color};
  Tensor scratch = at::empty({(int64_t)hgs_fsample_scratch_bytes((int32_t)M, in.num_blocks)}, opts.dtype(at::kByte));
  hgs_fsample_args a;
  memset(&a, 0, sizeof(a));
  a.info_host = &in;
  a.axis = fptr(ax);
  a.plan = plan.data_ptr();
  a.lists = lists.numel() ? lists.data_ptr() : nullptr;
  a.M = (int32_t)M;
  a.normalized = normalized ? 1 : 0;
  a.points = fptr(pts);
  a.colors = colors ? fptr(col) : nullptr;
  a.scratch = scratch.data_ptr();
  a.density = density.data_ptr<float>();
  a.normal = normal.data_ptr<float>();
  a.color = colors ? color->data_ptr<float>() : nullptr;
  check_rc(hgs_fsample(&a, c10::hip::getCurrentHIPStream(dev.index()).stream()), "hgs_fsample");
  return {density, normal, color};
}

// (vertices [V, 3] fp32 in index coordinates, triangles [T, 3] int32); one host wait for the two sizes
std::tuple<Tensor, Tensor> marching_cubes(const Tensor& field, double threshold) {
  at::NoGradGuard ng;
  const c10::Device dev = field.device();
  if (!dev.is_cuda()) throw std::runtime_error("humangaussian_amd: tensors must live on a HIP device");
  if (field.dim() != 3) throw std::runtime_error("field must have dimensions (X, Y, Z)");
  const auto opts = at::TensorOptions().device(dev);
  const int64_t X = field.size(0), Y = field.size(1), Z = field.size(2);
  if (X == 0 || Y == 0 || Z == 0)
    return {at::empty({0, 3}, opts.dtype(at::kFloat)), at::empty({0, 3}, opts.dtype(at::kInt))};
  if (X > (1 << 28) || Y > (1 << 28) || Z > (1 << 28)) throw std::runtime_error("marching_cubes: the field is too large");
  const size_t bytes = hgs_mc_scratch_bytes((int32_t)X, (int32_t)Y, (int32_t)Z);
  if (bytes == 0) throw std::runtime_error("marching_cubes: the field is too large (at most 2^28 samples)");
  DeviceSwitch guard(dev.index());
  const Tensor f = f32c(field, dev, "field");
  hipStream_t stream = c10::hip::getCurrentHIPStream(dev.index()).stream();
  Tensor scratch = at::empty({(int64_t)bytes}, opts.dtype(at::kByte));
  Tensor info_dev = at::empty({(int64_t)sizeof(hgs_mc_info)}, opts.dtype(at::kByte));
  auto* info_ptr = reinterpret_cast<hgs_mc_info*>(info_dev.data_ptr());
  check_rc(hgs_mc_count(fptr(f), (int32_t)X, (int32_t)Y, (int32_t)Z, (float)threshold, scratch.data_ptr(), info_ptr, stream),
           "hgs_mc_count");
  hgs_mc_info info;
  if (hipMemcpyAsync(&info, info_ptr, sizeof(info), hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess)
    throw std::runtime_error("marching_cubes: reading the sizes failed");
  Tensor v = at::empty({(int64_t)info.num_vertices, 3}, opts.dtype(at::kFloat));
  Tensor t = at::empty({(int64_t)info.num_triangles, 3}, opts.dtype(at::kInt));
  check_rc(hgs_mc_emit(fptr(f), (int32_t)X, (int32_t)Y, (int32_t)Z, (float)threshold, scratch.data_ptr(), &info,
                       info.num_vertices ? v.data_ptr<float>() : nullptr, info.num_triangles ? t.data_ptr<int32_t>() : nullptr,
                       stream), "hgs_mc_emit");
  return {v, t};
}

// ---- surface samples and the initial Gaussians (include/hgs_rast.h: hgs_surface_*, hgs_init_gaussians) --------------
// The table of a mesh: (cdf [F + 1] fp64, area, faces of positive area); one host wait, for the 16-byte info block.
std::tuple<Tensor, double, int64_t> surface_build(const Tensor& vertices, const Tensor& faces) {
  at::NoGradGuard ng;
  const c10::Device dev = vertices.device();
  if (!dev.is_cuda()) throw std::runtime_error("humangaussian_amd: tensors must live on a HIP device");
  DeviceSwitch guard(dev.index());
  const auto vf = mesh_inputs(vertices, faces, dev);
  const Tensor &v = vf.first, &f = vf.second;
  const int64_t V = v.size(0), F = f.size(0);
  if (F < 1 || F > HGS_SURFACE_MAX_FACES)
    throw std::runtime_error("surface_build: 1 .. " + std::to_string(HGS_SURFACE_MAX_FACES) + " faces, got " + std::to_string(F));
  const auto byte_opts = at::TensorOptions().dtype(at::kByte).device(dev);
  hipStream_t stream = c10::hip::getCurrentHIPStream(dev.index()).stream();
  Tensor cdf = at::empty({F + 1}, byte_opts.dtype(at::kDouble));
  Tensor scratch = at::empty({(int64_t)hgs_surface_cdf_scratch_bytes((int32_t)F)}, byte_opts);
  Tensor info_dev = at::empty({(int64_t)sizeof(hgs_surface_info)}, byte_opts);
  auto* info_ptr = reinterpret_cast<hgs_surface_info*>(info_dev.data_ptr());
  check_rc(hgs_surface_cdf((int32_t)V, fptr(v), (int32_t)F, f.data_ptr<int32_t>(), cdf.data_ptr<double>(), info_ptr,
                           scratch.data_ptr(), stream), "hgs_surface_cdf");
  hgs_surface_info info;
  if (hipMemcpyAsync(&info, info_ptr, sizeof(info), hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess)
    throw std::runtime_error("surface_build: reading the table's info block failed");
  return {cdf, info.area, (int64_t)info.num_positive};
}

// (points [N, 3] fp32, face [N] int32 or undefined, uvw [N, 3] fp32 or undefined): one launch, nothing read back
std::tuple<Tensor, c10::optional<Tensor>, c10::optional<Tensor>> surface_sample(
    const Tensor& vertices, const Tensor& faces, const Tensor& cdf, int64_t n, uint64_t seed, uint64_t offset, bool want_anchors) {
  at::NoGradGuard ng;
  const c10::Device dev = vertices.device();
  if (!dev.is_cuda()) throw std::runtime_error("humangaussian_amd: tensors must live on a HIP device");
  DeviceSwitch guard(dev.index());
  const auto vf = mesh_inputs(vertices, faces, dev);
  const Tensor &v = vf.first, &f = vf.second;
  const int64_t V = v.size(0), F = f.size(0);
  if (n < 0 || n > 0x7fffffffll / 3) throw std::runtime_error("surface_sample: 0 .. 715827882 samples a call");
  if (cdf.device() != dev || cdf.scalar_type() != at::kDouble || !cdf.is_contiguous() || cdf.numel() != F + 1)
    throw std::runtime_error("surface_sample: cdf is the (F + 1,) fp64 table surface_build returned for these faces");
  const auto opts = at::TensorOptions().device(dev).dtype(at::kFloat);
  Tensor points = at::empty({n, 3}, opts);
  c10::optional<Tensor> face, uvw;
  if (want_anchors) { face = at::empty({n}, opts.dtype(at::kInt)); uvw = at::empty({n, 3}, opts); }
  if (n == 0) return {points, face, uvw};
  hgs_surface_sample_args a;
  memset(&a, 0, sizeof(a));
  a.V = (int32_t)V; a.F = (int32_t)F;
  a.vertices = fptr(v); a.faces = f.data_ptr<int32_t>(); a.cdf = cdf.data_ptr<double>();
  a.N = n; a.offset = offset; a.seed = seed;
  a.points = points.data_ptr<float>();
  a.face = want_anchors ? face->data_ptr<int32_t>() : nullptr;
  a.uvw = want_anchors ? uvw->data_ptr<float>() : nullptr;
  check_rc(hgs_surface_sample(&a, c10::hip::getCurrentHIPStream(dev.index()).stream()), "hgs_surface_sample");
  return {points, face, uvw};
}

// create_from_pcd's tensors from distCUDA2's output: [features_dc (P,1,3), features_rest (P,M-1,3), scaling (P,3),
// rotation (P,4), opacity (P,1), max_radii2D (P)], one launch, nothing read back
std::vector<Tensor> init_gaussians(const Tensor& dist2, const c10::optional<Tensor>& colors, int64_t M) {
  at::NoGradGuard ng;
  const c10::Device dev = dist2.device();
  if (!dev.is_cuda()) throw std::runtime_error("humangaussian_amd: tensors must live on a HIP device");
  if (dist2.dim() != 1) throw std::runtime_error("dist2 must have dimensions (num_points,)");
  if (M < 1 || M > 4096) throw std::runtime_error("init_gaussians: M = (max_sh_degree + 1)^2 must be in 1 .. 4096");
  const int64_t P = dist2.size(0);
  if (colors && (colors->dim() != 2 || colors->size(0) != P || colors->size(1) != 3))
    throw std::runtime_error("colors must have dimensions (num_points, 3)");
  DeviceSwitch guard(dev.index());
  const Tensor d = f32c(dist2, dev, "dist2");
  Tensor col;
  if (colors) col = f32c(*colors, dev, "colors");
  const auto opts = at::TensorOptions().device(dev).dtype(at::kFloat);
  Tensor dc = at::empty({P, 1, 3}, opts), rest = at::empty({P, M - 1, 3}, opts), scaling = at::empty({P, 3}, opts),
         rotation = at::empty({P, 4}, opts), opacity = at::empty({P, 1}, opts), radii = at::empty({P}, opts);
  check_rc(hgs_init_gaussians(P, (int32_t)M, colors ? fptr(col) : nullptr, fptr(d), fptr_mut(dc), fptr_mut(rest),
                              fptr_mut(scaling), fptr_mut(rotation), fptr_mut(opacity), fptr_mut(radii),
                              c10::hip::getCurrentHIPStream(dev.index()).stream()), "hgs_init_gaussians");
  return {dc, rest, scaling, rotation, opacity, radii};
}

// ---- mesh view (include/hgs_rast.h: hgs_meshview_*): the body mesh rasterized forward-only on the current stream.
// vertices (Bv, V, 3) fp32 with Bv = 1 (one mesh for every view) or B, faces (F, 3) int32, mvp (B, 4, 4) fp32; everything
// contiguous on one device, nothing converted here.
namespace {
void mv_mesh_args(hgs_meshview_args& a, const Tensor& vertices, const Tensor& faces, int64_t B, const c10::Device& dev,
                  const char* who) {
  need_dev(vertices, dev, at::kFloat, who);
  need_dev(faces, dev, at::kInt, who);
  if (vertices.dim() != 3 || vertices.size(2) != 3) throw std::runtime_error(std::string(who) + ": vertices must be (Bv, V, 3)");
  if (faces.dim() != 2 || faces.size(1) != 3) throw std::runtime_error(std::string(who) + ": faces must be (F, 3)");
  const int64_t Bv = vertices.size(0), V = vertices.size(1), F = faces.size(0);
  if (Bv != 1 && Bv != B) throw std::runtime_error(std::string(who) + ": vertices must hold one mesh or one per view");
  if (B > 65535 || B * V >= 0x7fffffffll || B * F >= 0x7fffffffll || F > (1 << 24) - 1)
    throw std::runtime_error(std::string(who) + ": too many views, vertices or faces");
  a.B = (int32_t)B; a.V = (int32_t)V; a.F = (int32_t)F;
  a.vertex_stride = Bv == 1 ? 0 : 3 * V;
  a.vertices = fptr(vertices);
  a.faces = F > 0 ? faces.data_ptr<int32_t>() : nullptr;
}
void mv_attr_args(hgs_meshview_args& a, const Tensor& attr, const c10::Device& dev, const char* who) {
  need_dev(attr, dev, at::kFloat, who);
  if (attr.dim() != 3 || attr.size(1) != a.V || attr.size(2) < 1 || attr.size(2) > HGS_MESHVIEW_MAX_ATTR)
    throw std::runtime_error(std::string(who) + ": attr must be (Ba, V, C) with 1 <= C <= " + std::to_string(HGS_MESHVIEW_MAX_ATTR));
  if (attr.size(0) != 1 && attr.size(0) != a.B) throw std::runtime_error(std::string(who) + ": attr must hold one set or one per view");
  a.C = (int32_t)attr.size(2);
  a.attr_stride = attr.size(0) == 1 ? 0 : (int64_t)a.V * a.C;
  a.attr = fptr(attr);
}
}  // namespace

Tensor meshview_normals(const Tensor& vertices, const Tensor& faces, const Tensor& adj_start, const Tensor& adj) {
  at::NoGradGuard ng;
  const c10::Device dev = vertices.device();
  if (!dev.is_cuda()) throw std::runtime_error("humangaussian_amd: tensors must live on a HIP device");
  DeviceSwitch guard(dev.index());
  hgs_meshview_args a{};
  mv_mesh_args(a, vertices, faces, vertices.dim() == 3 ? vertices.size(0) : 1, dev, "meshview_normals");
  need_dev(adj_start, dev, at::kInt, "meshview_normals: adj_start");
  need_dev(adj, dev, at::kInt, "meshview_normals: adj");
  if (adj_start.numel() != (int64_t)a.V + 1 || adj.numel() != 3 * (int64_t)a.F)
    throw std::runtime_error("meshview_normals: adj_start must be (V + 1,) and adj (3 F,)");
  a.vertex_stride = 3 * (int64_t)a.V;
  a.adj_start = adj_start.data_ptr<int32_t>();
  a.adj = a.F > 0 ? adj.data_ptr<int32_t>() : nullptr;
  Tensor normals = at::empty({(int64_t)a.B, (int64_t)a.V, 3}, vertices.options());
  a.normals = fptr_mut(normals);
  check_rc(hgs_meshview_normals(&a, c10::hip::getCurrentHIPStream(dev.index()).stream()), "hgs_meshview_normals");
  return normals;
}

// (rast (B, H, W, 4) or None, image (B, H, W, C) or None, records (B, V, 4) int32).  attr None: rast alone.  attr (Ba, V, C):
// the image, shaded in the draw kernel, and rast too if want_rast.  One host wait (the plan's header sizes the lists).
std::tuple<c10::optional<Tensor>, c10::optional<Tensor>, Tensor> meshview_draw(
    const Tensor& vertices, const Tensor& mvp, const Tensor& faces, int64_t H, int64_t W, const c10::optional<Tensor>& attr,
    bool shade_normals, double background, bool want_rast) {
  at::NoGradGuard ng;
  const c10::Device dev = mvp.device();
  if (!dev.is_cuda()) throw std::runtime_error("humangaussian_amd: tensors must live on a HIP device");
  DeviceSwitch guard(dev.index());
  need_dev(mvp, dev, at::kFloat, "meshview_draw: mvp");
  if (mvp.dim() != 3 || mvp.size(1) != 4 || mvp.size(2) != 4) throw std::runtime_error("meshview_draw: mvp must be (B, 4, 4)");
  if (H < 1 || H > HGS_MESHVIEW_MAX_DIM || W < 1 || W > HGS_MESHVIEW_MAX_DIM)
    throw std::runtime_error("meshview_draw: H and W must be in [1, " + std::to_string(HGS_MESHVIEW_MAX_DIM) + "]");
  const int64_t B = mvp.size(0);
  hgs_meshview_args a{};
  mv_mesh_args(a, vertices, faces, B, dev, "meshview_draw");
  a.H = (int32_t)H; a.W = (int32_t)W;
  a.mvp = fptr(mvp);
  const bool shaded = attr.has_value() && attr->defined();
  if (shaded) {
    mv_attr_args(a, *attr, dev, "meshview_draw");
    if (shade_normals && a.C != 3) throw std::runtime_error("meshview_draw: normals have three channels");
    a.shade_normals = shade_normals ? 1 : 0;
    a.background = (float)background;
  }
  const auto opts = mvp.options();
  const int64_t V = a.V, C = a.C;
  Tensor records = at::empty({B, V, 4}, opts.dtype(at::kInt));
  c10::optional<Tensor> rast, image;
  const size_t plan_bytes = hgs_meshview_plan_bytes(a.B, a.F, a.H, a.W);
  if (plan_bytes == 0) throw std::runtime_error("meshview_draw: the sizes are outside the library's limits");
  hgs_meshview_info info{};
  hipStream_t stream = c10::hip::getCurrentHIPStream(dev.index()).stream();
  Tensor plan, info_dev, lists;
  if (B > 0) {
    plan = at::empty({(int64_t)plan_bytes}, opts.dtype(at::kByte));
    info_dev = at::empty({(int64_t)sizeof(hgs_meshview_info)}, opts.dtype(at::kByte));
    a.records = V > 0 ? records.data_ptr<int32_t>() : nullptr;
    a.plan = plan.data_ptr();
    a.info = reinterpret_cast<hgs_meshview_info*>(info_dev.data_ptr());
    check_rc(hgs_meshview_plan(&a, stream), "hgs_meshview_plan");
    if (hipMemcpyAsync(&info, a.info, sizeof(info), hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess)
      throw std::runtime_error("meshview_draw: reading the plan failed");
  }
  if (B == 0 || info.num_refs == 0) {            // nothing is listed: the background, without a draw
    if (!shaded || want_rast) rast = at::zeros({B, H, W, 4}, opts);
    if (shaded) image = at::full({B, H, W, C}, background, opts);
    return {rast, image, records};
  }
  const size_t bytes = hgs_meshview_list_bytes(&info);
  if (bytes == (size_t)-1)
    throw std::runtime_error("meshview_draw: " + std::to_string(info.num_refs) + " (triangle, tile) list entries; at most 2^31 - 1");
  lists = at::empty({(int64_t)bytes}, opts.dtype(at::kByte));
  a.lists = lists.data_ptr();
  if (!shaded || want_rast) { rast = at::empty({B, H, W, 4}, opts); a.rast = rast->data_ptr<float>(); }
  if (shaded) { image = at::empty({B, H, W, C}, opts); a.image = image->data_ptr<float>(); }
  check_rc(hgs_meshview_draw(&a, &info, stream), "hgs_meshview_draw");
  return {rast, image, records};
}

// attr (Ba, V, C), rast (B, H, W, 4), faces (F, 3) -> (B, H, W, C)
Tensor meshview_interpolate(const Tensor& attr, const Tensor& rast, const Tensor& faces) {
  at::NoGradGuard ng;
  const c10::Device dev = rast.device();
  if (!dev.is_cuda()) throw std::runtime_error("humangaussian_amd: tensors must live on a HIP device");
  DeviceSwitch guard(dev.index());
  need_dev(rast, dev, at::kFloat, "meshview_interpolate: rast");
  need_dev(faces, dev, at::kInt, "meshview_interpolate: faces");
  if (rast.dim() != 4 || rast.size(3) != 4) throw std::runtime_error("meshview_interpolate: rast must be (B, H, W, 4)");
  if (faces.dim() != 2 || faces.size(1) != 3) throw std::runtime_error("meshview_interpolate: faces must be (F, 3)");
  const int64_t B = rast.size(0), H = rast.size(1), W = rast.size(2), F = faces.size(0);
  if (H < 1 || H > HGS_MESHVIEW_MAX_DIM || W < 1 || W > HGS_MESHVIEW_MAX_DIM)
    throw std::runtime_error("meshview_interpolate: H and W must be in [1, " + std::to_string(HGS_MESHVIEW_MAX_DIM) + "]");
  if (attr.dim() != 3) throw std::runtime_error("meshview_interpolate: attr must be (Ba, V, C)");
  const int64_t V = attr.size(1);
  if (B > 65535 || B * V >= 0x7fffffffll || B * F >= 0x7fffffffll || F > (1 << 24) - 1)
    throw std::runtime_error("meshview_interpolate: too many views, vertices or faces");
  hgs_meshview_args a{};
  a.B = (int32_t)B; a.V = (int32_t)V; a.F = (int32_t)F; a.H = (int32_t)H; a.W = (int32_t)W;
  mv_attr_args(a, attr, dev, "meshview_interpolate");
  a.faces = F > 0 ? faces.data_ptr<int32_t>() : nullptr;
  a.rast_in = fptr(rast);
  Tensor image = at::empty({B, H, W, (int64_t)a.C}, rast.options());
  a.image = fptr_mut(image);
  if (B > 0 && (V == 0 || F == 0)) return image.zero_();
  check_rc(hgs_meshview_interpolate(&a, c10::hip::getCurrentHIPStream(dev.index()).stream()), "hgs_meshview_interpolate");
  return image;
}

// ---- mesh cleaning and decimation (include/hgs_rast.h: hgs_meshclean_*) -------------------------------------------------
namespace {
constexpr int MCL_ROUNDS_PER_READ = 4;     // component rounds launched between two host reads of their change counters

// one mesh's call state: the checked inputs, the scratch and the device info block
struct MclCall {
  c10::Device dev;
  Tensor v, f, scratch, info_dev, labels, comp_faces, comp_diag2;
  hgs_meshclean_args a{};
  hipStream_t stream = nullptr;
  std::unique_ptr<DeviceSwitch> guard;
  MclCall(const Tensor& vertices, const Tensor& faces, const char* who) : dev(vertices.device()) {
    if (!dev.is_cuda()) throw std::runtime_error("humangaussian_amd: tensors must live on a HIP device");
    guard.reset(new DeviceSwitch(dev.index()));
    if (vertices.dim() != 2 || vertices.size(1) != 3) throw std::runtime_error(std::string(who) + ": vertices must be (V, 3)");
    if (faces.dim() != 2 || faces.size(1) != 3) throw std::runtime_error(std::string(who) + ": faces must be (F, 3)");
    need_dev(faces, dev, at::kInt, "faces");
    if (vertices.size(0) > HGS_MESHCLEAN_MAX_ITEMS || faces.size(0) > HGS_MESHCLEAN_MAX_ITEMS)
      throw std::runtime_error(std::string(who) + ": at most 2^29 vertices and faces");
    v = f32c(vertices, dev, "vertices");
    f = faces.contiguous();
    a.V = (int32_t)v.size(0);
    a.F = (int32_t)f.size(0);
    const auto byte_opts = at::TensorOptions().dtype(at::kByte).device(dev);
    scratch = at::empty({(int64_t)hgs_meshclean_scratch_bytes(a.V, a.F)}, byte_opts);
    info_dev = at::empty({(int64_t)sizeof(hgs_meshclean_info)}, byte_opts);
    a.vertices = fptr(v);
    a.faces = a.F > 0 ? f.data_ptr<int32_t>() : nullptr;
    a.scratch = scratch.data_ptr();
    a.info = reinterpret_cast<hgs_meshclean_info*>(info_dev.data_ptr());
    stream = c10::hip::getCurrentHIPStream(dev.index()).stream();
  }
  void read(void* dst, const void* src, size_t bytes, const char* what) {
    if (hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
      throw std::runtime_error(std::string("humangaussian_amd: reading ") + what + " failed");
  }
  hgs_meshclean_info read_info() {
    hgs_meshclean_info info;
    read(&info, a.info, sizeof(info), "the mesh info block");
    if (info.error != 0)
      throw std::runtime_error("humangaussian_amd: a hash table of the mesh decimation ran into its probe bound (error " +
                               std::to_string(info.error) + ")");
    return info;
  }
  // labels, comp_faces, comp_diag2 of the mesh; returns {rounds, bad faces}.  One host read per MCL_ROUNDS_PER_READ rounds.
  std::pair<int64_t, int64_t> components() {
    const auto opts = at::TensorOptions().device(dev);
    labels = at::empty({(int64_t)a.V}, opts.dtype(at::kInt));
    comp_faces = at::empty({(int64_t)a.V}, opts.dtype(at::kInt));
    comp_diag2 = at::empty({(int64_t)a.V}, opts.dtype(at::kFloat));
    a.labels = a.V > 0 ? labels.data_ptr<int32_t>() : nullptr;
    a.comp_faces = a.V > 0 ? comp_faces.data_ptr<int32_t>() : nullptr;
    a.comp_diag2 = fptr_mut(comp_diag2);
    check_rc(hgs_meshclean_begin(&a, stream), "hgs_meshclean_begin");
    Tensor changed_dev = at::empty({MCL_ROUNDS_PER_READ}, opts.dtype(at::kInt));
    auto* changed_ptr = reinterpret_cast<uint32_t*>(changed_dev.data_ptr());
    const int64_t cap = (int64_t)a.V + 1 + MCL_ROUNDS_PER_READ;       // V + 1 rounds always suffice
    int64_t rounds = 0;
    for (bool settled = false; !settled;) {
      if (rounds >= cap)
        throw std::runtime_error("humangaussian_amd: the mesh components did not settle in " + std::to_string(cap) + " rounds");
      check_rc(hgs_meshclean_rounds(&a, MCL_ROUNDS_PER_READ, changed_ptr, stream), "hgs_meshclean_rounds");
      uint32_t changed[MCL_ROUNDS_PER_READ];
      read(changed, changed_ptr, sizeof(changed), "the component rounds' counters");
      for (int r = 0; r < MCL_ROUNDS_PER_READ && !settled; ++r) {
        ++rounds;
        settled = changed[r] == 0;
      }
    }
    check_rc(hgs_meshclean_components(&a, stream), "hgs_meshclean_components");
    hgs_meshclean_info info;
    read(&info, a.info, sizeof(info), "the mesh info block");
    return {rounds, (int64_t)info.bad_faces};
  }
  void no_bad_faces(const hgs_meshclean_info& info, const char* who) const {
    if (info.bad_faces != 0)
      throw std::runtime_error(std::string(who) + ": " + std::to_string(info.bad_faces) + " faces index vertices outside [0, " +
                               std::to_string(a.V) + ")");
  }
  // the output tensors of an emit call
  std::pair<Tensor, Tensor> outputs(const hgs_meshclean_info& info) {
    const auto opts = at::TensorOptions().device(dev);
    Tensor vo = at::empty({(int64_t)info.num_vertices, 3}, opts.dtype(at::kFloat));
    Tensor fo = at::empty({(int64_t)info.num_faces, 3}, opts.dtype(at::kInt));
    a.vertices_out = fptr_mut(vo);
    a.faces_out = info.num_faces > 0 ? fo.data_ptr<int32_t>() : nullptr;
    return {vo, fo};
  }
};

float mcl_key_float(uint32_t k) {       // gridscan.h::hgs_key_float on the host
  const uint32_t b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  float f;
  memcpy(&f, &b, 4);
  return f;
}
}  // namespace

// (labels [V] int32, comp_faces [V] int32, comp_diag2 [V] fp32, rounds, faces with an index out of range)
std::tuple<Tensor, Tensor, Tensor, int64_t, int64_t> meshclean_components(const Tensor& vertices, const Tensor& faces) {
  at::NoGradGuard ng;
  MclCall c(vertices, faces, "mesh_components");
  const auto rb = c.components();
  return {c.labels, c.comp_faces, c.comp_diag2, rb.first, rb.second};
}

// (vertices [V', 3], faces [F', 3] int32, vertex_src [V'] int32 or undefined, rounds)
std::tuple<Tensor, Tensor, c10::optional<Tensor>, int64_t> meshclean_clean(const Tensor& vertices, const Tensor& faces,
                                                                             int64_t min_f, double min_d, bool want_index) {
  at::NoGradGuard ng;
  MclCall c(vertices, faces, "clean_mesh");
  const auto rb = c.components();
  c.a.min_f = (int32_t)std::min<int64_t>(std::max<int64_t>(min_f, 0), 0x7fffffffll);
  c.a.min_d = (float)min_d;
  check_rc(hgs_meshclean_clean_mark(&c.a, c.stream), "hgs_meshclean_clean_mark");
  const hgs_meshclean_info info = c.read_info();
  c.no_bad_faces(info, "clean_mesh");
  const auto out = c.outputs(info);
  c10::optional<Tensor> vertex_src;
  if (want_index) {
    vertex_src = at::empty({(int64_t)info.num_vertices}, at::TensorOptions().device(c.dev).dtype(at::kInt));
    c.a.vertex_src = info.num_vertices > 0 ? vertex_src->data_ptr<int32_t>() : nullptr;
  }
  check_rc(hgs_meshclean_clean_emit(&c.a, &info, c.stream), "hgs_meshclean_clean_emit");
  return {out.first, out.second, vertex_src, rb.first};
}

// (vertices [V', 3], faces [F', 3] int32, g, cell edge, bisection launches): the caller has ruled out the no-op cases
std::tuple<Tensor, Tensor, int64_t, double, int64_t> meshclean_decimate(const Tensor& vertices, const Tensor& faces,
                                                                        int64_t target) {
  at::NoGradGuard ng;
  MclCall c(vertices, faces, "decimate_mesh");
  if (target < 0) throw std::runtime_error("decimate_mesh: the face budget must not be negative");
  check_rc(hgs_meshclean_begin(&c.a, c.stream), "hgs_meshclean_begin");
  Tensor counts_dev = at::empty({3}, at::TensorOptions().device(c.dev).dtype(at::kInt));
  auto* counts_ptr = reinterpret_cast<uint32_t*>(counts_dev.data_ptr());
  // the header's bisection, two steps per launch: mid and the two mids that can follow it
  int32_t lo = 1, hi = HGS_MESHCLEAN_G_MAX + 1;
  int64_t launches = 0;
  while (hi - lo > 1) {
    if (launches >= 10) throw std::runtime_error("decimate_mesh: the bisection did not end in 10 launches");
    const int32_t mid = (lo + hi) / 2, below = (lo + mid) / 2, above = (mid + hi) / 2;
    const int32_t g[3] = {mid, mid - lo > 1 ? below : 0, hi - mid > 1 ? above : 0};
    if (hipMemsetAsync(counts_ptr, 0, 12, c.stream) != hipSuccess) throw std::runtime_error("decimate_mesh: hipMemsetAsync failed");
    check_rc(hgs_meshclean_count(&c.a, g, counts_ptr, c.stream), "hgs_meshclean_count");
    uint32_t counts[3];
    c.read(counts, counts_ptr, sizeof(counts), "the surviving-face counts");
    ++launches;
    if ((int64_t)counts[0] <= target) {
      lo = mid;
      if (g[2] > 0) { if ((int64_t)counts[2] <= target) lo = above; else hi = above; }
    } else {
      hi = mid;
      if (g[1] > 0) { if ((int64_t)counts[1] <= target) lo = below; else hi = below; }
    }
  }
  check_rc(hgs_meshclean_decimate_mark(&c.a, lo, c.stream), "hgs_meshclean_decimate_mark");
  const hgs_meshclean_info info = c.read_info();
  c.no_bad_faces(info, "decimate_mesh");
  const auto out = c.outputs(info);
  check_rc(hgs_meshclean_decimate_emit(&c.a, &info, c.stream), "hgs_meshclean_decimate_emit");
  float emax = 0.0f;
  for (int k = 0; k < 3; ++k) emax = std::max(emax, mcl_key_float(info.bmax[k]) - mcl_key_float(info.bmin[k]));
  return {out.first, out.second, (int64_t)lo, (double)(emax / (float)lo), launches};
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "torch binding of libhgs_rast.so (include/hgs_rast.h): autograd node, capacity logic, the one host wait";
  m.def("rasterize", &rasterize, py::call_guard<py::gil_scoped_release>());
  m.def("rasterize_batch", &rasterize_batch, py::call_guard<py::gil_scoped_release>());
  m.def("mark_visible", &mark_visible, py::call_guard<py::gil_scoped_release>());
  m.def("knn_mean_dist2", &knn_mean_dist2, py::arg("points"), py::arg("brute_force") = false,
        py::call_guard<py::gil_scoped_release>());
  m.def("reduce_view_packs", &reduce_view_packs, py::arg("gathered"), py::arg("acc_in") = py::none(),
        py::call_guard<py::gil_scoped_release>());
  m.def("pack_view_contribution", &pack_view_contribution, py::call_guard<py::gil_scoped_release>());
  m.def("reduce_view_packs_unpack", &reduce_view_packs_unpack, py::arg("gathered"), py::arg("acc_in") = py::none(),
        py::call_guard<py::gil_scoped_release>());
  m.def("set_packed_backward", &set_packed_backward);
  m.def("take_packed", &take_packed);
  m.def("densify_stats", &densify_stats, py::call_guard<py::gil_scoped_release>());
  m.def("densify_masks", &densify_masks, py::call_guard<py::gil_scoped_release>());
  m.def("compact_rows", &compact_rows, py::call_guard<py::gil_scoped_release>());
  m.def("reanchor", &reanchor, py::call_guard<py::gil_scoped_release>());
  m.def("reanchor_rot", &reanchor_rot, py::call_guard<py::gil_scoped_release>());
  m.def("adam_step", &adam_step, py::arg("params"), py::arg("grads"), py::arg("exp_avgs"), py::arg("exp_avg_sqs"),
        py::arg("scalars"), py::arg("visible") = py::none(), py::call_guard<py::gil_scoped_release>());
  m.def("lbs_pose", &lbs_pose, py::arg("v_shaped"), py::arg("J_rest"), py::arg("parents"), py::arg("posedirs"),
        py::arg("weight_joint"), py::arg("weight_value"), py::arg("poses"), py::arg("transl") = py::none(),
        py::arg("centre") = std::vector<double>{0.0, 0.0, 0.0}, py::arg("scale") = 1.0, py::arg("return_joints") = false,
        py::call_guard<py::gil_scoped_release>());
  m.def("pose_draw", &pose_draw, py::arg("points"), py::arg("mvp"), py::arg("occlusion"), py::arg("style"), py::arg("H"),
        py::arg("W"), py::arg("limb_width"), py::arg("uint8_out") = false, py::call_guard<py::gil_scoped_release>());
  m.def("step_images_forward", &step_images_forward, py::arg("render"), py::arg("depth"), py::arg("h"), py::arg("w"),
        py::arg("half_images") = false, py::call_guard<py::gil_scoped_release>());
  m.def("step_images_backward", &step_images_backward, py::arg("depth"), py::arg("depth_min"), py::arg("depth_max"),
        py::arg("depth_global_max"), py::arg("tie_counts"), py::arg("h"), py::arg("w"), py::arg("half_images"),
        py::arg("grad_rgb") = py::none(), py::arg("grad_depth") = py::none(), py::arg("grad_loss_sparsity") = py::none(),
        py::arg("grad_loss_opaque") = py::none(), py::call_guard<py::gil_scoped_release>());
  m.def("photometric_forward", &photometric_forward, py::arg("image"), py::arg("gt"), py::arg("weight_l1"),
        py::arg("weight_dssim"), py::arg("psnr_per_plane") = false, py::arg("with_grad") = true,
        py::call_guard<py::gil_scoped_release>());
  m.def("photometric_backward", &photometric_backward, py::arg("image"), py::arg("gt"), py::arg("workspace"),
        py::arg("weight_l1"), py::arg("weight_dssim"), py::arg("grad_loss") = py::none(), py::arg("grad_l1") = py::none(),
        py::arg("grad_ssim") = py::none(), py::arg("grad_ssim_image") = py::none(), py::call_guard<py::gil_scoped_release>());
  m.def("mesh_build", &mesh_build,py::arg("vertices"), py::arg("faces"), py::call_guard<py::gil_scoped_release>());
  m.def("mesh_query", &mesh_query, py::arg("points"), py::arg("vertices"), py::arg("faces"), py::arg("grid") = py::none(),
        py::arg("raystab") = false, py::arg("want_uvw") = true, py::call_guard<py::gil_scoped_release>());
  m.def("field_extract", &field_extract, py::arg("xyz"), py::arg("opacity"), py::arg("scaling"), py::arg("rotation"),
        py::arg("axis"), py::arg("num_blocks"), py::arg("grow"), py::arg("want_counts") = false,
        py::call_guard<py::gil_scoped_release>());
  m.def("field_build", &field_build, py::arg("xyz"), py::arg("opacity"), py::arg("scaling"), py::arg("rotation"),
        py::arg("axis"), py::arg("num_blocks"), py::arg("grow"), py::arg("want_counts") = false,
        py::call_guard<py::gil_scoped_release>());
  m.def("field_sample", &field_sample, py::arg("info"), py::arg("axis"), py::arg("plan"), py::arg("lists"), py::arg("points"),
        py::arg("colors") = py::none(), py::arg("normalized") = false, py::call_guard<py::gil_scoped_release>());
  m.def("marching_cubes", &marching_cubes, py::arg("field"), py::arg("threshold"), py::call_guard<py::gil_scoped_release>());
  m.def("surface_build", &surface_build, py::arg("vertices"), py::arg("faces"), py::call_guard<py::gil_scoped_release>());
  m.def("surface_sample", &surface_sample, py::arg("vertices"), py::arg("faces"), py::arg("cdf"), py::arg("n"),
        py::arg("seed") = 0, py::arg("offset") = 0, py::arg("want_anchors") = false, py::call_guard<py::gil_scoped_release>());
  m.def("init_gaussians", &init_gaussians, py::arg("dist2"), py::arg("colors") = py::none(), py::arg("M") = 1,
        py::call_guard<py::gil_scoped_release>());
  m.def("meshview_normals", &meshview_normals, py::arg("vertices"), py::arg("faces"), py::arg("adj_start"), py::arg("adj"),
        py::call_guard<py::gil_scoped_release>());
  m.def("meshview_draw", &meshview_draw, py::arg("vertices"), py::arg("mvp"), py::arg("faces"), py::arg("H"), py::arg("W"),
        py::arg("attr") = py::none(), py::arg("shade_normals") = false, py::arg("background") = 0.0,
        py::arg("want_rast") = false, py::call_guard<py::gil_scoped_release>());
  m.def("meshview_interpolate", &meshview_interpolate, py::arg("attr"), py::arg("rast"), py::arg("faces"),
        py::call_guard<py::gil_scoped_release>());
  m.def("meshclean_components", &meshclean_components, py::arg("vertices"), py::arg("faces"),
        py::call_guard<py::gil_scoped_release>());
  m.def("meshclean_clean", &meshclean_clean, py::arg("vertices"), py::arg("faces"), py::arg("min_f"), py::arg("min_d"),
        py::arg("want_index") = false, py::call_guard<py::gil_scoped_release>());
  m.def("meshclean_decimate", &meshclean_decimate, py::arg("vertices"), py::arg("faces"), py::arg("target"),
        py::call_guard<py::gil_scoped_release>());
  m.def("set_stage_events", &set_stage_events);
  m.def("device_state", &device_state);
  m.def("abi_version", []() { return hgs_abi_version(); });
}
