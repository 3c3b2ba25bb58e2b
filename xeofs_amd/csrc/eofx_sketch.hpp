// eofx_sketch.hpp -- the Gaussian sketch generator of eofx_sketch_gaussian_f32, whole: host code only (threads, atomics, an AVX2
// recurrence), plain C++17 with no HIP in it, so the host compiler builds it alone (tests/test_sketch_cpu.py, and a stand-alone
// program under the thread and address sanitizers: tests/plans_shim.cpp).
#pragma once
#if !defined(__HIP_DEVICE_COMPILE__)
#include <immintrin.h>
#endif
#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include <pthread.h>
#include <sched.h>

namespace eofx_sketch {
// ------------------------------------------------------------------------------------
// Gaussian sketch matrix, bit-identical to numpy's legacy stream
//   np.random.RandomState(seed).normal(size=(rows, cols)).astype(np.float32)
// which is what scikit-learn draws for randomized_svd (extmath.py _randomized_range_finder), so
// `random_state` keeps its meaning.  MT19937 (init_genrand seeding), 53-bit doubles, Marsaglia
// polar method with the cached second deviate (numpy legacy_gauss).  The uniform stream and the
// accept/reject decisions are inherently sequential; the log/sqrt transforms of the accepted pairs
// are independent and run on worker threads (same libm, same results).
// ------------------------------------------------------------------------------------
// init_genrand seeding of the 624 state words
inline void mt_seed(uint32_t seed, uint32_t* mt) {
  mt[0] = seed;
  for (int i = 1; i < 624; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
}

// Parallel, still bit-identical.  Every candidate pair of the polar method consumes exactly four MT19937 words whether
// it is accepted or not, so candidate i always sits at words 4i..4i+3 of the stream.  Only the raw MT recurrence is
// sequential -- written as ONE linear recurrence x[i] = x[i-227] ^ f(x[i-624], x[i-623]) over the whole stream (no
// 624-word refill blocks, no copies), eight words per AVX2 step where the host has it: 0.55 ns per word on the GPU box,
// bound by one core's store bandwidth (40 MB for a 129 600 x 30 sketch).  Tempering, the conversion to doubles, the accept test and the log / sqrt of the accepted
// pairs are data-parallel over candidates: every worker thread turns its contiguous share of the candidates into its
// own list of deviates in ONE pass, and the lists are concatenated in order.
#define EOFX_MT_FILL_BODY                                                                                     \
  for (int64_t i = from; i < count; ++i) {                                                                     \
    const uint32_t y = (x[i - 624] & 0x80000000u) | (x[i - 623] & 0x7fffffffu);                               \
    x[i] = x[i - 227] ^ (y >> 1) ^ ((uint32_t)(-(int32_t)(y & 1u)) & 0x9908b0dfu);                            \
  }
#if !defined(__HIP_DEVICE_COMPILE__)
// eight words per step: every load lies at least 220 words behind the eight words being written.  [from, count): the
// words [0, from) are final (from >= 624), so the stream can be extended chunk by chunk.
__attribute__((target("avx2"))) inline void mt_fill_avx2_range(uint32_t* __restrict__ x, int64_t from, int64_t count) {
  const __m256i upper = _mm256_set1_epi32((int)0x80000000u), lower = _mm256_set1_epi32(0x7fffffff);
  const __m256i one = _mm256_set1_epi32(1), matrix = _mm256_set1_epi32((int)0x9908b0dfu), zero = _mm256_setzero_si256();
  int64_t i = from;
  for (; i + 8 <= count; i += 8) {
    const __m256i a = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(x + i - 624));
    const __m256i b = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(x + i - 623));
    const __m256i c = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(x + i - 227));
    const __m256i y = _mm256_or_si256(_mm256_and_si256(a, upper), _mm256_and_si256(b, lower));
    const __m256i mag = _mm256_and_si256(_mm256_sub_epi32(zero, _mm256_and_si256(y, one)), matrix);
    _mm256_storeu_si256(reinterpret_cast<__m256i*>(x + i), _mm256_xor_si256(_mm256_xor_si256(c, _mm256_srli_epi32(y, 1)), mag));
  }
  for (; i < count; ++i) {
    const uint32_t y = (x[i - 624] & 0x80000000u) | (x[i - 623] & 0x7fffffffu);
    x[i] = x[i - 227] ^ (y >> 1) ^ ((uint32_t)(-(int32_t)(y & 1u)) & 0x9908b0dfu);
  }
}
#else
inline void mt_fill_avx2_range(uint32_t*, int64_t, int64_t) {}   // (device pass of the single-source compile: host code only)
#endif
inline void mt_fill_generic_range(uint32_t* __restrict__ x, int64_t from, int64_t count) { EOFX_MT_FILL_BODY }
#undef EOFX_MT_FILL_BODY
inline uint32_t mt_temper(uint32_t y) {
  y ^= (y >> 11);
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= (y >> 18);
  return y;
}

// A small persistent pool for the data-parallel half of the sketch generator (starting a std::thread costs ~40 us; a
// 10000 x 60 sketch is ~1.5 ms of work in total, so eighteen fresh threads per call were a third of its wall time).
struct SketchPool {
  std::mutex mu;
  std::condition_variable cv_work, cv_done;
  std::vector<std::thread> threads;
  std::deque<std::function<void()>> tasks;
  int pending = 0;
  bool stop = false;
  void ensure(int n) {
    std::lock_guard<std::mutex> lk(mu);
    while ((int)threads.size() < n) threads.emplace_back([this] { loop(); });
  }
  // Keep the workers on the cores that share the calling thread's L3 (EOFX_SKETCH_PIN=1; Linux): the stream buffer then moves
  // between the producer and its consumers inside one cache instead of across the socket.
  int pinned_cpu = -1;
  int domain_threads = 0;     // hardware threads that share the caller's L3 (0: unknown / not pinned)
  void pin_near_caller() {
#if defined(__linux__) && !defined(__HIP_DEVICE_COMPILE__)
    const int cpu = sched_getcpu();
    if (cpu < 0 || cpu == pinned_cpu) return;
    char path[128];
    snprintf(path, sizeof(path), "/sys/devices/system/cpu/cpu%d/cache/index3/shared_cpu_list", cpu);
    FILE* f = fopen(path, "r");
    if (!f) return;
    char buf[512] = {0};
    const bool ok = fgets(buf, sizeof(buf), f) != nullptr;
    fclose(f);
    if (!ok) return;
    cpu_set_t set;
    CPU_ZERO(&set);
    int count = 0;
    for (char* tok = strtok(buf, ",\n"); tok; tok = strtok(nullptr, ",\n")) {
      int a = 0, b = 0;
      const int got = sscanf(tok, "%d-%d", &a, &b);
      if (got == 1) b = a;
      if (got < 1) continue;
      for (int c = a; c <= b && c < CPU_SETSIZE; ++c) { CPU_SET(c, &set); ++count; }
    }
    if (count < 2) return;
    std::lock_guard<std::mutex> lk(mu);
    for (auto& t : threads) (void)pthread_setaffinity_np(t.native_handle(), sizeof(set), &set);
    pinned_cpu = cpu;
    domain_threads = count;
#endif
  }
  void loop() {
    for (;;) {
      std::function<void()> job;
      {
        std::unique_lock<std::mutex> lk(mu);
        cv_work.wait(lk, [this] { return stop || !tasks.empty(); });
        if (stop && tasks.empty()) return;
        job = std::move(tasks.front());
        tasks.pop_front();
      }
      job();
      {
        std::lock_guard<std::mutex> lk(mu);
        if (--pending == 0) cv_done.notify_all();
      }
    }
  }
  void submit(std::function<void()> f) {
    {
      std::lock_guard<std::mutex> lk(mu);
      tasks.push_back(std::move(f));
      ++pending;
    }
    cv_work.notify_one();
  }
  void wait() {
    std::unique_lock<std::mutex> lk(mu);
    cv_done.wait(lk, [this] { return pending == 0; });
  }
  ~SketchPool() {
    {
      std::lock_guard<std::mutex> lk(mu);
      stop = true;
    }
    cv_work.notify_all();
    for (auto& t : threads) t.join();
  }
};
inline SketchPool& sketch_pool() {
  static SketchPool* pool = new SketchPool();     // leaked on purpose: worker threads must not be joined at exit order
  return *pool;
}
inline std::mutex g_sketch_call;    // one generation at a time (the pool's completion counter is per call)
// spin politely: a few thousand pauses (the waits here are microseconds), then give the core away -- on a host with fewer free
// cores than workers a pure spin would keep the producer off its core
struct SpinWait {
  int spins = 0;
  void operator()() {
#if !defined(__HIP_DEVICE_COMPILE__)
    if (++spins < 4000) _mm_pause();
    else std::this_thread::yield();
#endif
  }
};
// candidate pairs drawn in one round for `need` accepted ones: acceptance probability pi/4, ask for slightly more candidates
// than expected, at least a few (a round that accepts too few is followed by another)
inline int64_t candidates(int64_t need) { return (int64_t)((double)need / 0.7853981633974483 * 1.01) + 64; }

// out[rows x cols] (host), row-major: one draw of the stream (no memo)
inline void gaussian_f32_draw(uint32_t seed, int64_t rows, int64_t cols, float* out) {
  const int64_t total = rows * cols;
  if (total == 0) return;
  const int64_t npairs = (total + 1) / 2;
  const int hw = (int)std::thread::hardware_concurrency();
  // eight workers: the producer thread is the bound from four on (profiles/r04_sketch_probe.txt), and eight fit the physical cores
  // of one L3 domain, where the workers are kept (SketchPool::pin_near_caller)
  int max_threads = std::max(1, std::min(8, hw > 1 ? hw - 1 : 1));
  if (const char* ev = getenv("EOFX_SKETCH_THREADS")) max_threads = std::max(1, atoi(ev));
  static const bool have_avx2 = __builtin_cpu_supports("avx2");
  std::lock_guard<std::mutex> call_lock(g_sketch_call);
  // x[0..623]: the generator state (init_genrand seeding); x[624 + w]: raw (untempered) output word w of the stream
  uint32_t state[624];
  mt_seed(seed, state);
  int64_t done_pairs = 0;
  while (done_pairs < npairs) {
    const int64_t need = npairs - done_pairs;
    const int64_t ncand = candidates(need);
    const int64_t nwords = 4 * ncand;
    // ONE grow-only buffer for the process (calls are serialised by g_sketch_call): 40 MB of fresh pages per call cost
    // more than the recurrence itself -- and a buffer per calling THREAD meant exactly that for callers that draw on a
    // short-lived worker thread (engine.SketchFuture: 12 ms instead of 5.8 for the 129 600 x 30 sketch of config 3)
    static std::unique_ptr<uint32_t[]> xbuf;
    static size_t xcap = 0;
    if (xcap < (size_t)(624 + nwords)) {
      xbuf.reset(new uint32_t[(size_t)(624 + nwords)]);   // uninitialised on purpose
      xcap = (size_t)(624 + nwords);
    }
    uint32_t* x = xbuf.get();
    std::memcpy(x, state, sizeof(state));
    const uint32_t* raw = x + 624;
    // The raw recurrence is sequential and runs on this thread, chunk by chunk.  The workers are woken ONCE per call and
    // then claim chunks from an atomic counter, spinning (politely) for the few microseconds until the chunk they hold has
    // been produced: a mutex + condition-variable hand-over per 16 K-word chunk cost more than the chunk's recurrence.
    // Deviates go to one grow-only buffer at their chunk's place; once every chunk is done the same workers copy them to
    // their final offsets.
    const int64_t chunk = 4096;                                     // candidates per chunk (16 K words): the deviate work of the LAST chunk is the tail of the call
    const int64_t nchunks = (ncand + chunk - 1) / chunk;
    static std::unique_ptr<float[]> dbuf;                          // [nchunks][2 chunk]: (f b, f a) per accepted pair, in stream order
    static size_t dcap = 0;
    if (dcap < (size_t)(2 * chunk * nchunks)) {
      dbuf.reset(new float[(size_t)(2 * chunk * nchunks)]);
      dcap = (size_t)(2 * chunk * nchunks);
    }
    float* const dev = dbuf.get();
    std::vector<int64_t> cnt((size_t)nchunks, 0), off((size_t)nchunks + 1, 0);
    std::atomic<int64_t> produced{0}, claim{0}, finished{0}, claim2{0};
    std::atomic<int> phase2{0};
    auto work = [&](int64_t c) {
      const int64_t lo = c * chunk, hi = std::min<int64_t>(ncand, lo + chunk);
      float* d = dev + 2 * chunk * c;
      int64_t q = 0;
      for (int64_t i = lo; i < hi; ++i) {
        const uint32_t w0 = mt_temper(raw[4 * i]) >> 5, w1 = mt_temper(raw[4 * i + 1]) >> 6;
        const uint32_t w2 = mt_temper(raw[4 * i + 2]) >> 5, w3 = mt_temper(raw[4 * i + 3]) >> 6;
        const double a = 2.0 * ((w0 * 67108864.0 + w1) / 9007199254740992.0) - 1.0;
        const double b = 2.0 * ((w2 * 67108864.0 + w3) / 9007199254740992.0) - 1.0;
        const double r = a * a + b * b;
        if (r >= 1.0 || r == 0.0) continue;
        const double f = std::sqrt(-2.0 * std::log(r) / r);
        d[q++] = (float)(f * b);      // returned first
        d[q++] = (float)(f * a);      // the cached deviate
      }
      cnt[(size_t)c] = q;
    };
    const int64_t obase = 2 * done_pairs;
    auto copy_out = [&](int64_t c) {     // deviates beyond `total` belong to later draws of the stream and are dropped
      const int64_t o = obase + off[(size_t)c];
      if (o >= total) return;
      const int64_t take = std::min<int64_t>(cnt[(size_t)c], total - o);
      std::memcpy(out + o, dev + 2 * chunk * c, sizeof(float) * (size_t)take);
    };
    auto worker = [&] {
      for (;;) {
        const int64_t c = claim.fetch_add(1, std::memory_order_relaxed);
        if (c >= nchunks) break;
        for (SpinWait sw; produced.load(std::memory_order_acquire) <= c;) sw();
        work(c);
        finished.fetch_add(1, std::memory_order_release);
      }
      for (SpinWait sw; !phase2.load(std::memory_order_acquire);) sw();
      for (;;) {
        const int64_t c = claim2.fetch_add(1, std::memory_order_relaxed);
        if (c >= nchunks) break;
        copy_out(c);
      }
    };
    const int nworkers = (max_threads > 1 && nchunks > 1) ? (int)std::min<int64_t>(max_threads, nchunks) : 0;
    SketchPool& pool = sketch_pool();
    if (nworkers) {
      pool.ensure(nworkers);
      static const bool pin = !(getenv("EOFX_SKETCH_PIN") && atoi(getenv("EOFX_SKETCH_PIN")) == 0);
      if (pin) pool.pin_near_caller();
      for (int w = 0; w < nworkers; ++w) pool.submit(worker);
    }
    int64_t filled = 624;                                            // words of x that hold final values
    for (int64_t c = 0; c < nchunks; ++c) {
      const int64_t upto = 624 + 4 * std::min<int64_t>(ncand, (c + 1) * chunk);
      // the recurrence reads up to 624 words back and writes only beyond `filled`: extending the buffer in place
      if (have_avx2) mt_fill_avx2_range(x, filled, upto);
      else mt_fill_generic_range(x, filled, upto);
      filled = upto;
      produced.store(c + 1, std::memory_order_release);
    }
    for (;;) {                                                        // this thread takes chunks too once the stream stands
      const int64_t c = claim.fetch_add(1, std::memory_order_relaxed);
      if (c >= nchunks) break;
      work(c);
      finished.fetch_add(1, std::memory_order_release);
    }
    for (SpinWait sw; finished.load(std::memory_order_acquire) < nchunks;) sw();
    for (int64_t c = 0; c < nchunks; ++c) off[(size_t)c + 1] = off[(size_t)c] + cnt[(size_t)c];
    phase2.store(1, std::memory_order_release);
    for (;;) {
      const int64_t c = claim2.fetch_add(1, std::memory_order_relaxed);
      if (c >= nchunks) break;
      copy_out(c);
    }
    if (nworkers) pool.wait();
    std::memcpy(state, x + nwords, sizeof(state));     // the state after these words (a rare second round continues here)
    const int64_t o = std::min<int64_t>(total, obase + off[(size_t)nchunks]);
    done_pairs = (o + 1) / 2;
    if (o >= total) break;
  }
}

// The matrix depends on (seed, rows, cols) and nothing else, and a caller that fixes random_state and fits again and again (the
// Bootstrapper, fits over a moving window) asks for the same one every time: the last matrix drawn is kept, ONE entry for the
// process, and a hit is a copy (2.4 MB for the 10000 x 60 sketch against 0.58 ms of drawing).  Matrices above the cap are never kept.
constexpr size_t SKETCH_MEMO_MAX_BYTES = (size_t)64 << 20;
struct SketchMemo {
  std::mutex mu;
  bool valid = false;
  uint32_t seed = 0;
  int64_t rows = 0, cols = 0;
  std::vector<float> data;
};
inline SketchMemo& sketch_memo() {
  static SketchMemo* memo = new SketchMemo();     // leaked on purpose, like the pool: callers may outlive static destruction
  return *memo;
}
inline void sketch_memo_drop() {
  SketchMemo& mm = sketch_memo();
  std::lock_guard<std::mutex> lk(mm.mu);
  mm.valid = false;
  std::vector<float>().swap(mm.data);
}
// out[rows x cols] (host), row-major; safe under concurrent callers (a hit copies under the memo's lock, a miss draws outside it)
inline void gaussian_f32(uint32_t seed, int64_t rows, int64_t cols, float* out) {
  if (rows <= 0 || cols <= 0) return;
  const size_t total = (size_t)rows * (size_t)cols;
  const bool keep = total <= SKETCH_MEMO_MAX_BYTES / sizeof(float);
  SketchMemo& mm = sketch_memo();
  if (keep) {
    std::lock_guard<std::mutex> lk(mm.mu);
    if (mm.valid && mm.seed == seed && mm.rows == rows && mm.cols == cols) {
      std::memcpy(out, mm.data.data(), sizeof(float) * total);
      return;
    }
  }
  gaussian_f32_draw(seed, rows, cols, out);
  if (keep) {
    std::lock_guard<std::mutex> lk(mm.mu);
    mm.valid = false;
    mm.data.assign(out, out + total);
    mm.seed = seed;
    mm.rows = rows;
    mm.cols = cols;
    mm.valid = true;
  }
}

}  // namespace eofx_sketch
