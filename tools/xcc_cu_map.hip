// Which XCD (and shader engine / CU) each bit of a hipExtStreamCreateWithCUMask mask selects, and how the tail queue's
// mask (GpakSchedule::tail_mask CUs from bit 0, every tail_mask_stride-th) falls on the XCDs.  Every workgroup writes its
// HW_REG_XCC_ID and HW_REG_HW_ID through an ordinary vector store; nothing else runs.
//   hipcc -O2 --offload-arch=gfx950 tools/xcc_cu_map.hip -o tools/bin/xcc_cu_map && tools/bin/xcc_cu_map [skip stride]
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <tuple>
#include <vector>

#define CHECK(x)                                                                        \
  do {                                                                                  \
    hipError_t e_ = (x);                                                                \
    if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } \
  } while (0)

__global__ void where(int *out, int n) {
  if (threadIdx.x != 0 || (int)blockIdx.x >= n) return;
  const int xcc = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20);   // HW_REG_XCC_ID, bits 3:0
  const int hw = __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 4);    // HW_REG_HW_ID, all 32 bits
  out[2 * blockIdx.x] = xcc & 15;
  out[2 * blockIdx.x + 1] = hw;
  for (volatile int i = 0; i < 20000; i++) {}   // hold the slot a little so that the blocks spread over the allowed CUs
}

typedef std::tuple<int, int, int> Cu;   // xcc, se, cu (sh folded into cu)
static std::set<Cu> run(hipStream_t st, int *d, std::vector<int> &h, int blocks) {
  hipLaunchKernelGGL(where, dim3(blocks), dim3(64), 0, st, d, blocks);
  CHECK(hipStreamSynchronize(st));
  CHECK(hipMemcpy(h.data(), d, sizeof(int) * 2 * blocks, hipMemcpyDeviceToHost));
  std::set<Cu> s;
  for (int b = 0; b < blocks; b++) {
    const int hw = h[2 * b + 1];
    s.insert(Cu(h[2 * b], (hw >> 13) & 7, ((hw >> 12) & 1) * 16 + ((hw >> 8) & 15)));
  }
  return s;
}

int main(int argc, char **argv) {
  const int skip = argc > 1 ? atoi(argv[1]) : 8, stride = argc > 2 ? atoi(argv[2]) : 1;
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, 0));
  const int ncu = prop.multiProcessorCount, words = (ncu + 31) / 32, blocks = 2048;
  int *d = nullptr;
  CHECK(hipMalloc(&d, sizeof(int) * 2 * blocks));
  std::vector<int> h(2 * blocks);
  // every CU
  hipStream_t st;
  CHECK(hipStreamCreate(&st));
  const std::set<Cu> all = run(st, d, h, blocks);
  CHECK(hipStreamDestroy(st));
  std::map<int, int> per;
  for (auto &c : all) per[std::get<0>(c)]++;
  printf("all CUs: %zu seen;", all.size());
  for (auto &p : per) printf(" xcc%d:%d", p.first, p.second);
  printf("\n");
  // one mask bit at a time (the first 64 bits)
  printf("mask bit -> xcc se cu\n");
  for (int c = 0; c < 64 && c < ncu; c++) {
    std::vector<uint32_t> m(words, 0u);
    m[c / 32] = 1u << (c % 32);
    CHECK(hipExtStreamCreateWithCUMask(&st, (uint32_t)m.size(), m.data()));
    const std::set<Cu> s = run(st, d, h, 64);
    CHECK(hipStreamDestroy(st));
    printf("bit %3d ->", c);
    for (auto &x : s) printf(" (%d %d %d)", std::get<0>(x), std::get<1>(x), std::get<2>(x));
    printf("\n");
  }
  // the tail queue's mask
  std::vector<uint32_t> m(words, 0xffffffffu);
  for (int c = 0; c < skip; c++) { const int bit = (c * stride) % ncu; m[bit / 32] &= ~(1u << (bit % 32)); }
  CHECK(hipExtStreamCreateWithCUMask(&st, (uint32_t)m.size(), m.data()));
  const std::set<Cu> s = run(st, d, h, blocks);
  CHECK(hipStreamDestroy(st));
  std::map<int, int> pm;
  for (auto &c : s) pm[std::get<0>(c)]++;
  printf("tail mask (skip %d, stride %d): %zu CUs seen;", skip, stride, s.size());
  for (auto &p : pm) printf(" xcc%d:%d", p.first, p.second);
  printf("\n");
  CHECK(hipFree(d));
  return 0;
}
