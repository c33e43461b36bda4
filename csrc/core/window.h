// One-sided communication windows (MPI_Win_* equivalent, SURVEY §7.1 Tier 2).
//
// A device window is a region of HBM that every member rank maps through HIP IPC, so
// Put / Get are single hipMemcpyAsync peer copies over xGMI and Accumulate is a fused
// HIP kernel that read-modify-writes the remote HBM directly. A host window lives in a
// named POSIX shm object that every member maps. Each rank's window also carries a
// 64-B control block in host shm with a reader/writer lock word (Win_lock/Win_unlock).
//
// The parameter server (ps.h) is built on these windows: every client exposes an "rx"
// window (where pulled parameters land — normally the model's own flat parameter
// memory) and a "tx" window (pushed gradients / parameters), and servers read / write
// them directly, replacing the reference's message copies of whole shards
// (asyncsgd/pclient.lua:49-94, asyncsgd/pserver.lua:65-111).
#pragma once
#include <hip/hip_runtime.h>

#include <array>
#include <atomic>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "engine.h"

namespace mpit {

struct alignas(64) WinCtl {
  std::atomic<int64_t> lock;  // 0 free, >0 shared holders, -1 exclusive
  std::atomic<int64_t> epoch;
  char pad[48];
};

// A derived-datatype layout relative to a byte offset in a window (kernels.h type_copy: loops,
// run table, unit) and the bytes it touches, [lo, hi) relative to that offset.
struct CopyPlan {
  std::vector<std::array<int64_t, 2>> loops;
  uintptr_t table;  // on this rank's device for a device target, host memory for a host target
  int64_t R, L, per;
  int unit;
  int64_t lo, hi;
};

class Window {
 public:
  // local == 0 -> allocate `bytes` (hipMalloc for device windows, shm for host windows)
  Window(Engine& eng, int64_t id, uintptr_t local, int64_t bytes, bool device);
  ~Window();
  Window(const Window&) = delete;
  Window& operator=(const Window&) = delete;

  // this rank's exposure blob (exchange it among the members, then connect())
  std::string blob() const;
  // map_remote=false: leave other ranks' device windows unmapped (PS datapath 3 moves the
  // shard data as messages and never touches a peer allocation)
  void connect(const std::vector<std::string>& blobs, const std::vector<int>& world_ranks, bool map_remote = true);
  void unlink_names();  // after every member connected
  void check_alignment() const;

  uintptr_t local_ptr() const { return reinterpret_cast<uintptr_t>(local_); }
  int64_t bytes() const { return bytes_; }
  bool device() const { return device_; }
  int members() const { return int(remote_.size()); }
  uintptr_t remote_ptr(int m) const;  // member index
  int64_t remote_bytes(int m) const;
  bool remote_device(int m) const;

  // data movement (member index; offsets in bytes). src/dst device-ness given by caller.
  void put(int m, int64_t off, uintptr_t src, int64_t n, hipStream_t s);
  void get(uintptr_t dst, int m, int64_t off, int64_t n, hipStream_t s);
  // Put / Get with a derived target datatype in one type_copy launch: the layout `p` at byte
  // offset `off` of member m's window is the strided side (the peer-mapped pointer for a device
  // window, launched on s; the host twin for a host window), `packed` the local contiguous
  // stream (device memory for a device target, host memory for a host target). The plan's span
  // is checked against the target window (std::out_of_range, like put). Complete after flush(s).
  void put_plan(int m, int64_t off, const CopyPlan& p, uintptr_t packed, hipStream_t s);
  void get_plan(int m, int64_t off, const CopyPlan& p, uintptr_t packed, hipStream_t s);
  // dst[m][off..] = a*src + b*dst (fp32|bf16 elements), atomic w.r.t. other accumulates
  // through the exclusive lock of the target.
  void accumulate(int m, int64_t off, uintptr_t src, bool src_dev, int64_t nelem, bool bf16, float a, float b,
                  hipStream_t s);
  // Accumulate / Get_accumulate over a whole target layout in one type_accumulate launch
  // (kernels.h): for every element of the layout `p` at byte offset `off` of member m's window,
  // target = comb(op, target, packed) and, with fetch != 0, fetch = the target's previous element.
  // op: PeerOp / AccOp, dtype: PeerDtype. The plan's span is checked against the target window
  // as put_plan does (std::out_of_range, nothing launched, no lock taken). One exclusive target
  // lock, one launch on s (the host twin for a host window), one stream synchronise, unlock (on
  // a throw too): atomic w.r.t. other accumulates and complete on return. `packed` / `fetch` are
  // device memory for a device target and host memory for a host target.
  void accumulate_plan(int m, int64_t off, const CopyPlan& p, int op, int dtype, uintptr_t packed, uintptr_t fetch,
                       hipStream_t s);
  void lock(int m, bool exclusive);
  bool try_lock(int m, bool exclusive);
  void unlock(int m);
  void flush(hipStream_t s);  // complete all operations this rank issued on stream s

  // Barrier among this window's members only, on the per-rank epoch counters of the control
  // blocks (monotonic: bump mine with release, wait with acquire until every member's reached
  // it). Independent of Engine::barrier(), whose single world-wide counter pair another thread
  // of this rank may be inside at the same time. One thread per window at a time.
  void sync();
  // In-place all-reduce of nelem elements at byte offset `off` of every member's window
  // (kernels.h peer_reduce; member order = fold order, so the result is bitwise identical on
  // every rank). Blocking. mode: 0 = by size (MPIT_AR_ONESHOT_BYTES), 1 = one-shot, 2 = two-shot.
  // dst != 0: one-shot into that local buffer instead of the window (the window keeps the input).
  // Returns false, before any synchronisation, when this window cannot run it (more than 8
  // members, a member not mapped, mixed host / device members): the caller falls back.
  enum ArMode : int { kArAuto = 0, kArOneShot = 1, kArTwoShot = 2 };
  bool allreduce(int64_t off, int64_t nelem, int dtype, int op, hipStream_t s, int mode = kArAuto, uintptr_t dst = 0);
  bool allreduce_capable() const;
  static int64_t oneshot_bytes();  // MPIT_AR_ONESHOT_BYTES

  // The window collectives (kernels.h peer_gather / peer_fold / peer_scan). Each is blocking and
  // collective over the members, with allreduce's shape: stream synchronise, sync() (B1: inputs
  // complete everywhere), at most one kernel launch on this rank, stream synchronise, sync() (B2:
  // every read of my memory and every write into it has finished). Each returns false, before any
  // synchronisation, when allreduce_capable() is false, and throws on a range error before B1.
  // Local destinations are device memory for a device window and host memory for a host window.
  //
  // pull_gather: copy `bytes` bytes at byte offset `off` of member `member`'s window to `dst`,
  // for up to 8 segments in one launch (all-gather(v), all-to-all, broadcast). A segment that
  // names my own window at the address `dst` is dropped; an empty list takes part in the
  // barriers only.
  struct PullSeg {
    int member;
    int64_t off;
    uintptr_t dst;
    int64_t bytes;
  };
  bool pull_gather(const std::vector<PullSeg>& segs, hipStream_t s);
  // pull_plan: pull_gather between layouts, in one peer_plan_gather launch (kernels.h) for up to 8
  // segments: the layout `src` at byte offset `off` of member `member`'s window to the layout
  // `dstp` at the local address `dst` (Gatherv, Scatterv, Alltoallv, strided Alltoallw; a
  // contiguous side is the one-run plan). The two layouts of a segment have the same packed size
  // (std::invalid_argument) and the source span lies inside the member's window
  // (std::out_of_range); both are checked, with all the kernel checks its arguments, before B1.
  // The segment's unit is the largest power of two <= 16 dividing both base addresses, every
  // stride, L and per of both sides and both plans' `unit` (what the caller knows to divide the
  // offsets of their tables). An empty segment is dropped, as is my own window at the address and
  // layout of `dst`; an empty list takes part in the barriers only. Tables are on this rank's
  // device for a device window, in host memory for a host window (the host twin).
  struct PlanPull {
    int member;
    int64_t off;
    CopyPlan src;
    uintptr_t dst;
    CopyPlan dstp;
  };
  bool pull_plan(const std::vector<PlanPull>& segs, hipStream_t s);
  // pull_fold: dst[i] = fold over members [m0, m1) in member order of element i of the nelem
  // elements at byte offset `off` of their windows (reduce-scatter: every rank its own segment;
  // rooted reduce: the root alone). dst == 0 or nelem == 0: the barriers only.
  bool pull_fold(int64_t off, int64_t nelem, int dtype, int op, uintptr_t dst, int m0, int m1, hipStream_t s);
  // scan: in place at byte offset `off` of every member's window, member j ends with the fold of
  // members 0..j (exclusive: 0..j-1, member 0's window untouched). Two-shot like allreduce: rank r
  // loads slice r (the same 16-byte-rounded bounds) from all members and stores prefix j into
  // member j, so every rank reads and writes the range once whatever the member count.
  bool scan(int64_t off, int64_t nelem, int dtype, int op, bool exclusive, hipStream_t s);

 private:
  Engine& eng_;
  int64_t id_;
  int64_t bytes_;
  bool device_;
  bool own_ = false;
  void* local_ = nullptr;
  std::string ctl_name_;
  WinCtl* ctl_ = nullptr;
  void* ctl_map_ = nullptr;
  int64_t ctl_map_bytes_ = 0;
  struct Remote {
    void* ptr = nullptr;
    int64_t bytes = 0;
    bool device = false;
    int world_rank = -1;
    int align = 0;  // the owner's base address mod 16, from its blob (the same on every rank)
    WinCtl* ctl = nullptr;
    void* map = nullptr;
    int64_t map_bytes = 0;
  };
  std::vector<Remote> remote_;
  std::vector<int> held_;  // lock mode held per member: 0 none, 1 shared, 2 exclusive
  // the span check of a plan against member m's window; the strided base address, 0 for an empty plan
  uintptr_t plan_base(int m, int64_t off, const CopyPlan& p, const char* outside) const;
  void copy_plan(int dir, int m, int64_t off, const CopyPlan& p, uintptr_t packed, hipStream_t s);
  int self_member(const char* who = "collective") const;  // my index among the members (throws when I am none)
  // One epoch of a window collective: select the device, drain the stream, sync() (B1), launch(dev)
  // with dev = -1 for a host window, drain, sync() (B2). Callers validate and throw before it;
  // `launch` does not throw on validated arguments.
  void epoch(hipStream_t s, const char* what, const std::function<void(int)>& launch);
  // bound k of the n slices of a range, the same on every rank (two-shot all-reduce, scan)
  int64_t slice_bounds(int k, int n, int64_t nelem, int64_t off, int64_t es) const;
  // the range check of the reducing collectives, in two parts: aligned for dtype (invalid_argument),
  // and inside the window of every member in [m0, m1) (out_of_range)
  void check_range_aligned(const char* who, int64_t off, int64_t nelem, int dtype) const;
  void check_range_inside(const char* who, int64_t off, int64_t nelem, int dtype, int m0, int m1) const;
  std::vector<uintptr_t> member_ptrs(int64_t off, int m0, int m1) const;  // members' window bases + off
  void* ar_tmp_ = nullptr;  // one-shot in place: the private result, copied back after B2
  int64_t ar_tmp_bytes_ = 0;
};

}  // namespace mpit
