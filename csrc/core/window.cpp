#include "window.h"

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <xmmintrin.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <new>
#include <stdexcept>
#include <thread>

#include "../kernels/kernels.h"

namespace mpit {

namespace {

void hipw(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string("mpit window HIP error in ") + what + ": " + hipGetErrorString(e));
}

struct Blob {
  int64_t bytes;
  int32_t device;
  int32_t world_rank;
  int32_t align;  // base address mod 16 in the owner's address space
  int64_t offset;
  hipIpcMemHandle_t handle;
  char ctl_name[160];
};

void* map_named(const std::string& name, int64_t bytes, bool create) {
  int fd;
  if (create) {
    ::shm_unlink(name.c_str());
    fd = ::shm_open(name.c_str(), O_CREAT | O_EXCL | O_RDWR, 0600);
    if (fd < 0) throw std::runtime_error("mpit: window shm_open(create) failed: " + name);
    if (::ftruncate(fd, bytes) != 0) {
      ::close(fd);
      throw std::runtime_error("mpit: window ftruncate failed");
    }
  } else {
    fd = ::shm_open(name.c_str(), O_RDWR, 0600);
    if (fd < 0) throw std::runtime_error("mpit: window shm_open(attach) failed: " + name);
  }
  void* p = ::mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
  ::close(fd);
  if (p == MAP_FAILED) throw std::runtime_error("mpit: window mmap failed");
  return p;
}

constexpr int64_t kCtl = 64;

}  // namespace

Window::Window(Engine& eng, int64_t id, uintptr_t local, int64_t bytes, bool device)
    : eng_(eng), id_(id), bytes_(bytes), device_(device) {
  if (device && eng.device() < 0) throw std::invalid_argument("mpit: device window on a rank without a device");
  ctl_name_ = eng.seg().name() + "_w" + std::to_string(id) + "_r" + std::to_string(eng.rank());
  ctl_map_bytes_ = kCtl + (device ? 0 : std::max<int64_t>(bytes, 0));
  ctl_map_ = map_named(ctl_name_, std::max<int64_t>(ctl_map_bytes_, 64), true);
  ctl_ = new (ctl_map_) WinCtl();
  ctl_->lock.store(0);
  ctl_->epoch.store(0);
  if (device) {
    if (local) {
      local_ = reinterpret_cast<void*>(local);
    } else if (bytes > 0) {
      hipw(hipSetDevice(eng.device()), "hipSetDevice");
      hipw(hipMalloc(&local_, size_t(bytes)), "hipMalloc(window)");
      hipw(hipMemset(local_, 0, size_t(bytes)), "hipMemset(window)");
      own_ = true;
    }
  } else {
    local_ = static_cast<uint8_t*>(ctl_map_) + kCtl;
    if (local && bytes > 0) std::memcpy(local_, reinterpret_cast<const void*>(local), size_t(bytes));
  }
}

Window::~Window() {
  for (auto& r : remote_)
    if (r.map && r.map != ctl_map_) ::munmap(r.map, std::max<int64_t>(r.map_bytes, 64));
  if (ctl_map_) ::munmap(ctl_map_, std::max<int64_t>(ctl_map_bytes_, 64));
  ::shm_unlink(ctl_name_.c_str());
  if (ar_tmp_) {
    if (device_) {
      hipSetDevice(eng_.device());
      hipFree(ar_tmp_);
    } else {
      std::free(ar_tmp_);
    }
  }
  if (own_ && local_) {
    hipSetDevice(eng_.device());
    hipFree(local_);
  }
}

std::string Window::blob() const {
  Blob b{};
  b.bytes = bytes_;
  b.device = device_ ? 1 : 0;
  b.world_rank = eng_.rank();
  b.align = int32_t(reinterpret_cast<uintptr_t>(local_) & 15);
  std::strncpy(b.ctl_name, ctl_name_.c_str(), sizeof(b.ctl_name) - 1);
  if (device_ && local_ && bytes_ > 0) {
    hipw(hipSetDevice(eng_.device()), "hipSetDevice");
    Engine::export_ptr(local_, &b.handle, &b.offset, nullptr);
  }
  return std::string(reinterpret_cast<const char*>(&b), sizeof(b));
}

void Window::connect(const std::vector<std::string>& blobs, const std::vector<int>& world_ranks, bool map_remote) {
  remote_.assign(blobs.size(), Remote{});
  held_.assign(blobs.size(), 0);
  for (size_t m = 0; m < blobs.size(); ++m) {
    if (blobs[m].size() != sizeof(Blob)) throw std::invalid_argument("mpit: bad window blob");
    Blob b;
    std::memcpy(&b, blobs[m].data(), sizeof(b));
    Remote& r = remote_[m];
    r.bytes = b.bytes;
    r.device = b.device != 0;
    r.world_rank = b.world_rank;
    r.align = b.align;
    if (world_ranks.size() == blobs.size() && world_ranks[m] != b.world_rank)
      throw std::invalid_argument("mpit: window member order mismatch");
    if (b.world_rank == eng_.rank()) {
      r.ptr = local_;
      r.ctl = ctl_;
      r.map = ctl_map_;
      continue;
    }
    r.map_bytes = kCtl + (r.device ? 0 : std::max<int64_t>(b.bytes, 0));
    r.map = map_named(b.ctl_name, std::max<int64_t>(r.map_bytes, 64), false);
    r.ctl = static_cast<WinCtl*>(r.map);
    if (!r.device) {
      r.ptr = static_cast<uint8_t*>(r.map) + kCtl;
    } else if (b.bytes > 0 && eng_.device() >= 0 && map_remote) {
      try {
        r.ptr = static_cast<uint8_t*>(eng_.open_ipc(b.world_rank, b.handle)) + b.offset;
      } catch (const std::exception& e) {
        // name the pair: which rank (device) could not map whose window (device)
        throw std::runtime_error("mpit: rank " + std::to_string(eng_.rank()) + " (device " +
                                 std::to_string(eng_.device()) + ") could not map window " + std::to_string(id_) +
                                 " of rank " + std::to_string(b.world_rank) + ": " + e.what());
      }
    }
  }
  check_alignment();
}

// Window::allreduce cuts its slices at 16-byte addresses computed from the
// owners' published alignment; a mapping that does not keep it would make ranks disagree.
void Window::check_alignment() const {
  for (const Remote& r : remote_)
    if (r.ptr && int(reinterpret_cast<uintptr_t>(r.ptr) & 15) != r.align)
      throw std::runtime_error("mpit: window " + std::to_string(id_) + " of rank " + std::to_string(r.world_rank) +
                               " is mapped at another 16-byte alignment than its owner's");
}

void Window::unlink_names() { ::shm_unlink(ctl_name_.c_str()); }

uintptr_t Window::remote_ptr(int m) const { return reinterpret_cast<uintptr_t>(remote_.at(size_t(m)).ptr); }
int64_t Window::remote_bytes(int m) const { return remote_.at(size_t(m)).bytes; }
bool Window::remote_device(int m) const { return remote_.at(size_t(m)).device; }

void Window::put(int m, int64_t off, uintptr_t src, int64_t n, hipStream_t s) {
  const Remote& r = remote_.at(size_t(m));
  if (off < 0 || off + n > r.bytes) throw std::out_of_range("mpit: Put outside the target window");
  if (!r.ptr && n > 0) throw std::runtime_error("mpit: target window not mapped on this rank");
  uint8_t* dst = static_cast<uint8_t*>(r.ptr) + off;
  if (eng_.device() >= 0) {
    hipw(hipSetDevice(eng_.device()), "hipSetDevice");
    hipw(hipMemcpyAsync(dst, reinterpret_cast<const void*>(src), size_t(n), hipMemcpyDefault, s), "Put");
  } else {
    std::memcpy(dst, reinterpret_cast<const void*>(src), size_t(n));
  }
}

void Window::get(uintptr_t dst, int m, int64_t off, int64_t n, hipStream_t s) {
  const Remote& r = remote_.at(size_t(m));
  if (off < 0 || off + n > r.bytes) throw std::out_of_range("mpit: Get outside the target window");
  if (!r.ptr && n > 0) throw std::runtime_error("mpit: target window not mapped on this rank");
  const uint8_t* src = static_cast<const uint8_t*>(r.ptr) + off;
  if (eng_.device() >= 0) {
    hipw(hipSetDevice(eng_.device()), "hipSetDevice");
    hipw(hipMemcpyAsync(reinterpret_cast<void*>(dst), src, size_t(n), hipMemcpyDefault, s), "Get");
  } else {
    std::memcpy(reinterpret_cast<void*>(dst), src, size_t(n));
  }
}

uintptr_t Window::plan_base(int m, int64_t off, const CopyPlan& p, const char* outside) const {
  const Remote& r = remote_.at(size_t(m));
  if (p.lo > p.hi) throw std::invalid_argument("mpit: one-sided plan with lo > hi");
  if (p.hi == p.lo) return 0;  // nothing to move
  if (off < 0 || off + p.lo < 0 || off + p.hi > r.bytes) throw std::out_of_range(outside);
  if (!r.ptr) throw std::runtime_error("mpit: target window not mapped on this rank");
  return reinterpret_cast<uintptr_t>(r.ptr) + uintptr_t(off);
}

void Window::copy_plan(int dir, int m, int64_t off, const CopyPlan& p, uintptr_t packed, hipStream_t s) {
  const Remote& r = remote_.at(size_t(m));
  const uintptr_t strided =
      plan_base(m, off, p, dir ? "mpit: Put outside the target window" : "mpit: Get outside the target window");
  if (!strided) return;
  if (r.device) {
    if (eng_.device() < 0) throw std::runtime_error("mpit: device target window on a rank without a device");
    type_copy(eng_.device(), s, dir, strided, packed, p.loops, p.table, p.R, p.L, p.per, p.unit);
  } else {
    type_copy(-1, nullptr, dir, strided, packed, p.loops, p.table, p.R, p.L, p.per, p.unit);
  }
}

void Window::put_plan(int m, int64_t off, const CopyPlan& p, uintptr_t packed, hipStream_t s) {
  copy_plan(1, m, off, p, packed, s);
}

void Window::get_plan(int m, int64_t off, const CopyPlan& p, uintptr_t packed, hipStream_t s) {
  copy_plan(0, m, off, p, packed, s);
}

void Window::accumulate(int m, int64_t off, uintptr_t src, bool src_dev, int64_t nelem, bool bf16, float a, float b,
                        hipStream_t s) {
  const Remote& r = remote_.at(size_t(m));
  const int64_t es = bf16 ? 2 : 4;
  if (off < 0 || off + nelem * es > r.bytes) throw std::out_of_range("mpit: Accumulate outside the target window");
  uint8_t* dst = static_cast<uint8_t*>(r.ptr) + off;
  lock(m, true);
  try {
    const uint32_t bf = bf16 ? 3u : 0u;
    if (r.device) {
      if (!src_dev) throw std::invalid_argument("mpit: Accumulate into a device window needs a device origin buffer");
      ew_update(kAxpby, 0, eng_.device(), s, nelem, {reinterpret_cast<uintptr_t>(dst), src}, bf, {a, b});
      hipw(hipStreamSynchronize(s), "Accumulate sync");
    } else {
      if (src_dev) throw std::invalid_argument("mpit: Accumulate into a host window needs a host origin buffer");
      ew_update(kAxpby, 0, -1, nullptr, nelem, {reinterpret_cast<uintptr_t>(dst), src}, bf, {a, b});
    }
  } catch (...) {
    unlock(m);
    throw;
  }
  unlock(m);
}

namespace {
// whether `p` is device memory, asked of the runtime (only on a rank that has a device; plain
// host memory is unknown to it, which is an error there and not one here)
bool device_memory(uintptr_t p) {
  hipPointerAttribute_t at{};
  if (hipPointerGetAttributes(&at, reinterpret_cast<const void*>(p)) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return at.type == hipMemoryTypeDevice;
}
}  // namespace

void Window::accumulate_plan(int m, int64_t off, const CopyPlan& p, int op, int dtype, uintptr_t packed,
                             uintptr_t fetch, hipStream_t s) {
  const Remote& r = remote_.at(size_t(m));
  const uintptr_t strided = plan_base(m, off, p, "mpit: Accumulate outside the target window");
  if (!strided) return;
  if (!type_accumulate_supported(op, dtype)) throw std::invalid_argument("mpit: Accumulate: unsupported (op, dtype)");
  if (r.device && eng_.device() < 0) throw std::runtime_error("mpit: device target window on a rank without a device");
  if (eng_.device() >= 0) {
    hipw(hipSetDevice(eng_.device()), "hipSetDevice");
    for (uintptr_t q : {packed, fetch}) {
      if (!q) continue;
      const bool dev = device_memory(q);
      if (r.device && !dev)
        throw std::invalid_argument("mpit: Accumulate into a device window needs device origin and result buffers");
      if (!r.device && dev)
        throw std::invalid_argument("mpit: Accumulate into a host window needs host origin and result buffers");
    }
  }
  lock(m, true);
  try {
    if (r.device) {
      type_accumulate(eng_.device(), s, op, dtype, strided, packed, fetch, p.loops, p.table, p.R, p.L, p.per, p.unit);
      hipw(hipStreamSynchronize(s), "Accumulate sync");
    } else {
      type_accumulate(-1, nullptr, op, dtype, strided, packed, fetch, p.loops, p.table, p.R, p.L, p.per, p.unit);
    }
  } catch (...) {
    unlock(m);
    throw;
  }
  unlock(m);
}

bool Window::try_lock(int m, bool exclusive) {
  WinCtl* c = remote_.at(size_t(m)).ctl;
  int64_t v = c->lock.load(std::memory_order_acquire);
  if (exclusive) {
    int64_t z = 0;
    if (c->lock.compare_exchange_strong(z, -1, std::memory_order_acq_rel)) {
      held_[size_t(m)] = 2;
      return true;
    }
    return false;
  }
  if (v < 0) return false;
  if (c->lock.compare_exchange_strong(v, v + 1, std::memory_order_acq_rel)) {
    held_[size_t(m)] = 1;
    return true;
  }
  return false;
}

void Window::lock(int m, bool exclusive) {
  int spins = 0;
  while (!try_lock(m, exclusive)) {
    if (++spins < 1000) _mm_pause();
    else std::this_thread::sleep_for(std::chrono::microseconds(5));
  }
}

void Window::unlock(int m) {
  WinCtl* c = remote_.at(size_t(m)).ctl;
  const int h = held_.at(size_t(m));
  if (h == 2) c->lock.store(0, std::memory_order_release);
  else if (h == 1) c->lock.fetch_sub(1, std::memory_order_acq_rel);
  else throw std::runtime_error("mpit: Win_unlock without a matching Win_lock");
  held_[size_t(m)] = 0;
}

void Window::flush(hipStream_t s) {
  if (eng_.device() >= 0) {
    hipw(hipSetDevice(eng_.device()), "hipSetDevice");
    hipw(hipStreamSynchronize(s), "Win_flush");
  }
}

void Window::sync() {
  const int64_t mine = ctl_->epoch.fetch_add(1, std::memory_order_release) + 1;
  const double tmo = Engine::wait_timeout_s();
  const auto t0 = std::chrono::steady_clock::now();
  for (const Remote& r : remote_) {
    if (r.ctl == ctl_) continue;
    int spins = 0;
    while (r.ctl->epoch.load(std::memory_order_acquire) < mine) {
      eng_.poll_abort();
      if (++spins < 2000) {
        _mm_pause();
      } else if (spins < 2256) {
        std::this_thread::yield();
      } else {
        std::this_thread::sleep_for(std::chrono::microseconds(20));
        if (tmo > 0 && (spins & 255) == 0 &&
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > tmo)
          eng_.fatal("window " + std::to_string(id_) + " sync timed out after " + std::to_string(int(tmo)) +
                     " s waiting for rank " + std::to_string(r.world_rank) + " (MPIT_WAIT_TIMEOUT_S)");
      }
    }
  }
}

int64_t Window::oneshot_bytes() {
  // Default 0: two-shot at every size. With the ranks sharing one GPU (all this pool can
  // measure, profiles/win_allreduce.md) one-shot never wins: it reads n times the bytes and
  // pays a copy-back after the second barrier. Across distinct GPUs a small message may
  // prefer it (one hop less); set the crossover measured there.
  const char* e = std::getenv("MPIT_AR_ONESHOT_BYTES");
  return e && *e ? std::atoll(e) : 0;
}

bool Window::allreduce_capable() const {
  if (remote_.empty() || remote_.size() > size_t(kPeerMax)) return false;
  for (const Remote& r : remote_)
    if (r.device != device_ || (r.bytes > 0 && !r.ptr)) return false;
  return true;
}

// The epoch every window collective runs its one launch in. Between the two barriers nothing may
// throw (a rank that left would leave the others waiting): the callers validate their arguments
// and throw before they come here, and `launch(dev)` does not throw on validated arguments.
void Window::epoch(hipStream_t s, const char* what, const std::function<void(int)>& launch) {
  const int dev = device_ ? eng_.device() : -1;
  auto drain = [&](const char* barrier) {
    if (dev >= 0) hipw(hipStreamSynchronize(s), (std::string(what) + barrier).c_str());
  };
  if (dev >= 0) hipw(hipSetDevice(dev), "hipSetDevice");
  drain(" B1");
  sync();  // B1: every member's input is complete
  launch(dev);
  drain(" B2");
  sync();  // B2: every result has landed at its owner and every read of my memory is finished
}

// Bound k of the n slices of nelem elements at byte offset off (two-shot all-reduce, scan).
// Interior bounds are rounded down to a 16-B address of member 0's range, from the alignment
// member 0 published in its blob (checked against every mapping at connect), so every rank
// computes the same bounds. They count elements, so a slice never starts inside a pair.
int64_t Window::slice_bounds(int k, int n, int64_t nelem, int64_t off, int64_t es) const {
  if (k <= 0) return 0;
  if (k >= n) return nelem;
  const int64_t b = nelem * k / n;
  const int64_t a = ((int64_t(remote_[0].align) + off + b * es) & 15) / es;
  return std::max<int64_t>(0, b - a);
}

// a reducing collective's range: aligned for dtype ...
void Window::check_range_aligned(const char* who, int64_t off, int64_t nelem, int dtype) const {
  if (off < 0 || nelem < 0 || off % peer_dtype_align(dtype))
    throw std::invalid_argument(std::string("mpit: ") + who + " range misaligned");
}

// ... and inside the window of every member in [m0, m1)
void Window::check_range_inside(const char* who, int64_t off, int64_t nelem, int dtype, int m0, int m1) const {
  for (int m = m0; m < m1; ++m)
    if (off + nelem * peer_dtype_size(dtype) > remote_[size_t(m)].bytes)
      throw std::out_of_range(std::string("mpit: ") + who + " range outside a member's window");
}

std::vector<uintptr_t> Window::member_ptrs(int64_t off, int m0, int m1) const {
  std::vector<uintptr_t> p;
  for (int m = m0; m < m1; ++m) p.push_back(reinterpret_cast<uintptr_t>(remote_[size_t(m)].ptr) + uintptr_t(off));
  return p;
}

bool Window::allreduce(int64_t off, int64_t nelem, int dtype, int op, hipStream_t s, int mode, uintptr_t dst) {
  if (!allreduce_capable() || !peer_reduce_supported(op, dtype)) return false;
  const int64_t es = peer_dtype_size(dtype);  // a pair type: nelem counts pairs, es is the pair's extent
  const int n = int(remote_.size());
  check_range_aligned("window all-reduce", off, nelem, dtype);
  check_range_inside("all-reduce", off, nelem, dtype, 0, n);
  const int dev = device_ ? eng_.device() : -1;
  const int me = self_member("all-reduce");
  const bool oneshot = dst != 0 || mode == kArOneShot || (mode == kArAuto && nelem * es <= oneshot_bytes());
  // two-shot push: rank r reduces slice r (slice_bounds) from all members and stores it into all
  // members. One-shot: every rank reduces the whole range. My window must stay as it is until B2
  // (a slower peer may still be reading it): the result goes to `dst`, or to a private buffer
  // copied back after B2.
  const int64_t lo = oneshot ? 0 : slice_bounds(me, n, nelem, off, es);
  const int64_t hi = oneshot ? nelem : slice_bounds(me + 1, n, nelem, off, es);
  const std::vector<uintptr_t> srcs = member_ptrs(off + lo * es, 0, n);
  std::vector<uintptr_t> dsts = srcs;
  if (oneshot && nelem > 0) {
    if (!dst && ar_tmp_bytes_ < nelem * es) {  // (before B1: nothing throws between the barriers)
      if (dev >= 0) hipw(hipSetDevice(dev), "hipSetDevice");
      if (ar_tmp_) {
        if (dev >= 0) hipw(hipFree(ar_tmp_), "hipFree(all-reduce tmp)");
        else std::free(ar_tmp_);
        ar_tmp_ = nullptr;
      }
      const int64_t cap = std::max<int64_t>(nelem * es, 64 << 10);
      if (dev >= 0) hipw(hipMalloc(&ar_tmp_, size_t(cap)), "hipMalloc(all-reduce tmp)");
      else if (!(ar_tmp_ = std::malloc(size_t(cap)))) throw std::bad_alloc();
      ar_tmp_bytes_ = cap;
    }
    dsts = {dst ? dst : reinterpret_cast<uintptr_t>(ar_tmp_)};
  }
  epoch(s, "all-reduce", [&](int d) {
    if (hi > lo) peer_reduce(d, s, op, dtype, srcs, dsts, hi - lo);
  });
  if (nelem > 0 && oneshot && !dst) {
    void* mine = reinterpret_cast<void*>(srcs[size_t(me)]);
    if (dev >= 0) {
      hipw(hipMemcpyAsync(mine, ar_tmp_, size_t(nelem * es), hipMemcpyDeviceToDevice, s), "all-reduce copy back");
      hipw(hipStreamSynchronize(s), "all-reduce copy back");
    } else {
      std::memcpy(mine, ar_tmp_, size_t(nelem * es));
    }
  }
  return true;
}

int Window::self_member(const char* who) const {
  for (size_t m = 0; m < remote_.size(); ++m)
    if (remote_[m].ctl == ctl_) return int(m);
  throw std::runtime_error(std::string("mpit: window ") + who + " on a rank that is no member");
}

bool Window::pull_gather(const std::vector<PullSeg>& segs, hipStream_t s) {
  if (!allreduce_capable()) return false;
  if (segs.size() > size_t(kPeerMax)) throw std::invalid_argument("mpit: pull-gather takes up to 8 segments");
  self_member();
  std::vector<uintptr_t> srcs, dsts;
  std::vector<int64_t> bytes;
  for (const PullSeg& g : segs) {
    if (g.member < 0 || g.member >= int(remote_.size())) throw std::out_of_range("mpit: pull-gather member out of range");
    const Remote& r = remote_[size_t(g.member)];
    if (g.off < 0 || g.bytes < 0 || g.off + g.bytes > r.bytes)
      throw std::out_of_range("mpit: pull-gather range outside a member's window");
    if (g.bytes == 0) continue;
    if (!g.dst) throw std::invalid_argument("mpit: pull-gather without a destination");
    srcs.push_back(reinterpret_cast<uintptr_t>(r.ptr) + uintptr_t(g.off));
    dsts.push_back(g.dst);
    bytes.push_back(g.bytes);
  }
  epoch(s, "pull-gather", [&](int dev) {
    if (!srcs.empty()) peer_gather(dev, s, srcs, dsts, bytes);
  });
  return true;
}

bool Window::pull_plan(const std::vector<PlanPull>& segs, hipStream_t s) {
  if (!allreduce_capable()) return false;
  if (segs.size() > size_t(kPeerMax)) throw std::invalid_argument("mpit: pull-plan takes up to 8 segments");
  self_member();
  // the low bits of everything the host knows of a plan (the table's offsets are the caller's: p.unit)
  auto bits_of = [](const CopyPlan& p) {
    uint64_t b = uint64_t(p.L) | uint64_t(p.per) | uint64_t(p.unit);
    for (const auto& l : p.loops)
      if (l[0] > 1) b |= uint64_t(l[1]);
    return b;
  };
  std::vector<PlanSegment> plan;
  for (const PlanPull& g : segs) {
    if (g.member < 0 || g.member >= int(remote_.size())) throw std::out_of_range("mpit: pull-plan member out of range");
    const uintptr_t base = plan_base(g.member, g.off, g.src, "mpit: pull-plan source outside a member's window");
    if (g.dstp.lo > g.dstp.hi) throw std::invalid_argument("mpit: pull-plan destination plan with lo > hi");
    if ((base == 0) != (g.dstp.lo == g.dstp.hi))
      throw std::invalid_argument("mpit: pull-plan: the two sides of a segment differ in packed size");
    if (!base) continue;  // nothing to move
    if (!g.dst) throw std::invalid_argument("mpit: pull-plan without a destination");
    const uint64_t b = bits_of(g.src) | bits_of(g.dstp) | uint64_t(base) | uint64_t(g.dst) | 16u;
    PlanSegment sg;
    sg.src = PlanSide{base, g.src.loops, g.src.table, g.src.R, g.src.L, g.src.per};
    sg.dst = PlanSide{g.dst, g.dstp.loops, g.dstp.table, g.dstp.R, g.dstp.L, g.dstp.per};
    sg.unit = int(b & (~b + 1));
    plan.push_back(std::move(sg));
  }
  peer_plan_check(plan);  // (throws here, never between the barriers)
  epoch(s, "pull-plan", [&](int dev) {
    if (!plan.empty()) peer_plan_gather(dev, s, plan);
  });
  return true;
}

bool Window::pull_fold(int64_t off, int64_t nelem, int dtype, int op, uintptr_t dst, int m0, int m1, hipStream_t s) {
  if (!allreduce_capable() || !peer_reduce_supported(op, dtype)) return false;
  check_range_aligned("pull-fold", off, nelem, dtype);
  if (m0 < 0 || m1 > int(remote_.size()) || m0 >= m1) throw std::out_of_range("mpit: pull-fold member range");
  if (dst % uintptr_t(peer_dtype_align(dtype))) throw std::invalid_argument("mpit: pull-fold destination misaligned");
  self_member();
  const bool reads = dst && nelem > 0;  // otherwise this rank only keeps the epoch: no member is read
  if (reads) check_range_inside("pull-fold", off, nelem, dtype, m0, m1);
  const std::vector<uintptr_t> srcs = member_ptrs(off, m0, reads ? m1 : m0);
  epoch(s, "pull-fold", [&](int dev) {
    if (!srcs.empty()) peer_fold(dev, s, op, dtype, srcs, dst, nelem);
  });
  return true;
}

bool Window::scan(int64_t off, int64_t nelem, int dtype, int op, bool exclusive, hipStream_t s) {
  if (!allreduce_capable() || !peer_reduce_supported(op, dtype)) return false;
  const int64_t es = peer_dtype_size(dtype);
  const int n = int(remote_.size());
  check_range_aligned("window scan", off, nelem, dtype);
  check_range_inside("scan", off, nelem, dtype, 0, n);
  const int me = self_member();
  // the slices of Window::allreduce's two-shot
  const int64_t lo = slice_bounds(me, n, nelem, off, es), hi = slice_bounds(me + 1, n, nelem, off, es);
  const std::vector<uintptr_t> sl = member_ptrs(off + lo * es, 0, n);
  epoch(s, "scan", [&](int dev) {
    if (hi > lo) peer_scan(dev, s, op, dtype, exclusive, sl, sl, hi - lo);
  });
  return true;
}

}  // namespace mpit
