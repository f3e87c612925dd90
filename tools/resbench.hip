// Micro-benchmark: what the memory system does with k_scatter32's region reservations.  The scatter's 256 persistent
// workgroups of 1024 threads each do, once per tile, one returning device-scope atomicAdd per thread on
// cursor[partition] — 1024 consecutive words, sixty-four 64-byte lines that every workgroup hits.  Here: G workgroups
// of 1024 threads, every round each thread does `reps` returning adds on cur[s·1024 + threadIdx.x] with
// s = blockIdx.x % S (S "segments" of cursors: S = 1 is the scatter's layout), either back to back or PACED — a chain
// of dependent VALU work of ≈ `pace_us` between the rounds (the scatter's tile cadence is ≈ 8 µs), a barrier per
// round like the scatter's.  A wave's instruction covers 256 B = four lines, so a line gets G/S · reps requests per
// round.  Reported: µs per round, the time a wave waits for its returned values (issue of the first add → last value
// in a register), and requests per µs per line.  nt = 512 with G = 512 is the two-workgroups-per-CU shape: half the
// threads, two adds per thread to cover the 1024 words, twice the requests per line and round.
//   resbench [G=256] [rounds=2000] [reps=1] [pace_us=8] [nt=1024]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#define CK(x) do { hipError_t e=(x); if(e!=hipSuccess){printf("err %s line %d\n", hipGetErrorString(e), __LINE__); exit(1);} } while(0)
constexpr int NT = 1024, P = 1024, S_MAX = 16;

__global__ void __launch_bounds__(NT) k_res(unsigned int *cur, uint32_t S, uint32_t rounds, uint32_t reps, uint32_t pace,
                                            uint32_t *sink, unsigned long long *wait_ticks) {
  const uint32_t per = P / blockDim.x;  // cursor words per thread
  uint32_t acc = threadIdx.x;
  unsigned int *w = cur + (blockIdx.x % S) * P + threadIdx.x;
  unsigned long long waited = 0;
  for (uint32_t r = 0; r < rounds; ++r) {
    for (uint32_t i = 0; i < pace; ++i) acc = acc * 1664525u + 1013904223u;  // dependent: nothing to overlap inside a wave
    const unsigned long long t0 = wall_clock64();
    uint32_t g = 0;
    for (uint32_t j = 0; j < reps; ++j)
      for (uint32_t q = 0; q < per; ++q) g += atomicAdd(w + q * blockDim.x, (acc & 1u) + 1u);  // issued back to back, all returning
    acc ^= g;
    asm volatile("" : "+v"(acc));  // the values are in registers before the clock is read
    waited += wall_clock64() - t0;
    __syncthreads();
  }
  if ((threadIdx.x & 63) == 0) atomicAdd(wait_ticks, waited);
  if (acc == 12345u) sink[0] = acc;
}

static uint32_t g_nt = NT;
static float run(unsigned int *cur, uint32_t G, uint32_t S, uint32_t rounds, uint32_t reps, uint32_t pace, uint32_t *sink,
                 unsigned long long *d_wait, double *wait_us) {
  hipEvent_t a, b;
  CK(hipEventCreate(&a));
  CK(hipEventCreate(&b));
  float best = 1e9f;
  for (int it = 0; it < 4; ++it) {
    CK(hipMemset(cur, 0, (size_t)S_MAX * P * 4));
    CK(hipMemset(d_wait, 0, 8));
    CK(hipEventRecord(a));
    hipLaunchKernelGGL(k_res, dim3(G), dim3(g_nt), 0, 0, cur, S, rounds, reps, pace, sink, d_wait);
    CK(hipEventRecord(b));
    CK(hipEventSynchronize(b));
    float ms;
    CK(hipEventElapsedTime(&ms, a, b));
    if (ms < best) {
      best = ms;
      unsigned long long wt;
      CK(hipMemcpy(&wt, d_wait, 8, hipMemcpyDeviceToHost));
      // wall_clock64 ticks at 100 MHz: 0.01 µs; mean over the launch's waves and rounds
      if (wait_us) *wait_us = (double)wt * 0.01 / ((double)G * (g_nt / 64) * rounds);
    }
  }
  CK(hipEventDestroy(a));
  CK(hipEventDestroy(b));
  return best;
}

int main(int argc, char **argv) {
  const uint32_t G = argc > 1 ? atoi(argv[1]) : 256;
  const uint32_t rounds = argc > 2 ? atoi(argv[2]) : 2000;
  const uint32_t reps = argc > 3 ? atoi(argv[3]) : 1;
  const double pace_us = argc > 4 ? atof(argv[4]) : 8.0;
  g_nt = argc > 5 && atoi(argv[5]) == 512 ? 512 : NT;
  unsigned int *cur;
  uint32_t *sink;
  unsigned long long *d_wait;
  CK(hipMalloc(&cur, (size_t)S_MAX * P * 4));
  CK(hipMalloc(&sink, 4));
  CK(hipMalloc(&d_wait, 8));
  // how many links of the chain make pace_us (no atomics: reps = 0)
  const uint32_t probe = 4000;
  const float ms0 = run(cur, G, 1, 200, 0, probe, sink, d_wait, nullptr);
  const double us_per_link = ms0 * 1e3 / 200.0 / probe;
  const uint32_t pace = (uint32_t)(pace_us / us_per_link + 0.5);
  const float ms1 = run(cur, G, 1, rounds, 0, pace, sink, d_wait, nullptr);
  const double pace_round = ms1 * 1e3 / rounds;
  printf("G=%u workgroups x %u threads, %u rounds, %u returning adds per thread and round; pace: %u links = %.2f us per round without atomics\n",
         G, g_nt, rounds, reps, pace, pace_round);
  printf("%-6s %-3s %12s %14s %14s %22s\n", "mode", "S", "us/round", "over pace us", "wave wait us", "requests/us/line");
  for (int paced = 0; paced < 2; ++paced)
    for (uint32_t S = 1; S <= (uint32_t)S_MAX; S *= 2) {
      double wait_us = 0;
      const float ms = run(cur, G, S, rounds, reps, paced ? pace : 0, sink, d_wait, &wait_us);
      const double us_round = ms * 1e3 / rounds;
      const double per_line = (double)((G + S - 1) / S) * reps;  // requests a line gets per round
      printf("%-6s %-3u %12.3f %14.3f %14.3f %22.1f\n", paced ? "paced" : "b2b", S, us_round, paced ? us_round - pace_round : us_round, wait_us,
             per_line / us_round);
    }
  return 0;
}
