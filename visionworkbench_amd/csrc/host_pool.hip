// host_pool.hip — the helper threads of a context.
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

#include "vwgpu_internal.h"

// ---- helper threads of a context ----------------------------------------------------------------------------------------
// The host side of a tile group is per-tile work on tables the device sent back (the zone scheduler's accept / retry / merge walk, the zone
// task lists of the next level: ~30 000 zones for 16 tiles at level 0, milliseconds on one thread with the device idle).  A context keeps a
// few helper threads for it: persistent (the zone scheduler caches its trees per thread), parked on a condition variable between jobs.
namespace {
struct HostPool {
  std::vector<std::thread> workers;
  std::mutex m;
  std::condition_variable wake, done;
  void (*fn)(void*, int) = nullptr;
  void* arg = nullptr;
  int n = 0;
  std::atomic<int> next{0};
  int running = 0;                   // workers still inside the current job
  unsigned long long job = 0;        // generation counter
  bool quit = false;
  void work() {
    for (;;) {
      const int i = next.fetch_add(1);
      if (i >= n) return;
      fn(arg, i);
    }
  }
  void loop() {
    unsigned long long seen = 0;
    for (;;) {
      {
        std::unique_lock<std::mutex> lk(m);
        wake.wait(lk, [&] { return quit || job != seen; });
        if (quit) return;
        seen = job;
      }
      work();
      {
        std::lock_guard<std::mutex> lk(m);
        if (--running == 0) done.notify_one();
      }
    }
  }
};
}  // namespace

void vwgpu_pool_run(vwgpu_ctx* ctx, int n, void (*fn)(void*, int), void* arg) {
  if (n <= 0) return;
  HostPool* P = static_cast<HostPool*>(ctx->host_pool);
  if (!P && n >= 4) {
    P = new HostPool();
    const unsigned hc = std::thread::hardware_concurrency();
    const int nw = hc >= 32 ? 7 : (hc >= 8 ? 3 : 0);               // + the calling thread
    for (int i = 0; i < nw; ++i) P->workers.emplace_back([P] { P->loop(); });
    ctx->host_pool = P;
  }
  if (!P || P->workers.empty() || n < 4) { for (int i = 0; i < n; ++i) fn(arg, i); return; }
  {
    std::lock_guard<std::mutex> lk(P->m);
    P->fn = fn; P->arg = arg; P->n = n; P->next.store(0);
    P->running = (int)P->workers.size();
    ++P->job;
  }
  P->wake.notify_all();
  P->work();
  std::unique_lock<std::mutex> lk(P->m);
  P->done.wait(lk, [&] { return P->running == 0; });
}

void vwgpu_pool_destroy(vwgpu_ctx* ctx) {
  HostPool* P = static_cast<HostPool*>(ctx->host_pool);
  if (!P) return;
  {
    std::lock_guard<std::mutex> lk(P->m);
    P->quit = true;
  }
  P->wake.notify_all();
  for (std::thread& t : P->workers) t.join();
  delete P;
  ctx->host_pool = nullptr;
}
