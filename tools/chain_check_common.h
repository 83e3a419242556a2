// Shared by the host-only checks of the chain entry points (tools/chain_args_check.cpp, tools/chain2_side_args_check.cpp): the library's
// error text and launch check stubbed, the kernel launch replaced by a recorder, dummy operands that are never dereferenced.
#pragma once
#include <hip/hip_runtime.h>

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "common.h"

namespace anemoi {
static char g_err[512];
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}
int check_launch(const char*) { return ANEMOI_OK; }
}  // namespace anemoi

// One recorded launch.  kernel: the instantiation as the host code names it, its dtype argument dropped ("gt_chain2_kernel<false,true>").
struct Record {
  std::string kernel;
  int grid = 0, block = 0, smem = 0;
  int n_rows = 0, rows_per_tile = 0, n_tiles = 0;
  long long row_begin = 0;  // panel ranges: the first row of the shifted job
  int pipe = -1, host_grid = 0, first = 0, end = 0, riders = 0, side_tiles = 0;
};
static std::vector<Record> g_launches;

static std::string kernel_name(const char* text) {
  std::string s;
  for (const char* c = text; *c; ++c)
    if (*c != '(' && *c != ')' && *c != ' ') s += *c;
  for (const char* t : {"<T>", "<bf16_t>", "<f16_t>"})
    if (size_t at = s.find(t); at != std::string::npos) s.erase(at, strlen(t));
  for (const char* t : {"<T,", "<bf16_t,", "<f16_t,"})
    if (size_t at = s.find(t); at != std::string::npos) s.replace(at, strlen(t), "<");
  return s;
}

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, smem, stream, arg) record_launch(#kernel, (grid), (block), (smem), (arg))
#define hipFuncSetAttribute(...) hipSuccess

static int g_fail = 0, g_cases = 0;
#define EXPECT(cond, ...)                                   \
  do {                                                      \
    ++g_cases;                                              \
    if (!(cond)) {                                          \
      ++g_fail;                                             \
      printf("FAIL line %d: %s  ", __LINE__, #cond);        \
      printf(__VA_ARGS__);                                  \
      printf("  [%s]\n", anemoi::g_err);                    \
    }                                                       \
  } while (0)

static void* P(uintptr_t v) { return reinterpret_cast<void*>(v); }  // aligned dummy addresses: never dereferenced on the host

static anemoi_gt_chain2_args_t host_block(int n_rows, int q_out, int hidden = 2048, int rows_per_tile = 0) {
  anemoi_gt_chain2_args_t a;
  memset(&a, 0, sizeof a);
  a.attn = P(0x10000); a.ld_attn = 512; a.x_res = P(0x20000); a.ld_x = 512;
  a.wp = P(0x30000); a.w1 = P(0x40000); a.hidden = hidden; a.w2 = P(0x50000);
  a.wq = q_out ? P(0x60000) : nullptr; a.q_out_features = q_out; a.vec = P(0x70000);
  a.ln1_eps = a.lnq_eps = 1e-5f;
  a.x_out = P(0x80000); a.ld_out = 512; a.q_out = q_out ? P(0x90000) : nullptr; a.ld_q = q_out;
  a.n_rows = n_rows; a.channels = 512; a.rows_per_tile = rows_per_tile;
  return a;
}
constexpr uintptr_t kRowChainX = 0xa0000000;
static anemoi_gt_rowchain_args_t side_block(int n_rows, int k_in, int q_out, int rows_per_tile = 0) {
  anemoi_gt_rowchain_args_t s;
  memset(&s, 0, sizeof s);
  s.x = P(kRowChainX); s.ld_x = k_in; s.in_features = k_in; s.we = P(0xb0000); s.wq = P(0xc0000); s.q_out_features = q_out;
  s.vec = P(0xd0000); s.ln_eps = 1e-5f; s.x_out = P(0xe0000); s.ld_out = 512; s.q_out = P(0xf0000); s.ld_q = q_out;
  s.n_rows = n_rows; s.channels = 512; s.rows_per_tile = rows_per_tile;
  return s;
}

// One row of the recorded table (tests/golden/chain_plan_recorded.json): the call, the return code, the launch (null: none).
static void print_row(const char* kind, std::initializer_list<long long> call, int rc, const Record* r, bool tail_alone = false) {
  printf("[\"%s\", [", kind);
  const char* sep = "";
  for (long long v : call) printf("%s%lld", sep, v), sep = ", ";
  printf("], %d, ", rc);
  if (tail_alone) printf("\"tail_alone\"]\n");
  else if (r == nullptr) printf("null]\n");
  else
    printf("[\"%s\", %d, %d, %d, %d, %d, %d, %lld, %d, %d, %d, %d, %d]]\n", r->kernel.c_str(), r->grid, r->block, r->smem, r->rows_per_tile, r->n_tiles,
           r->n_rows, r->row_begin, r->host_grid, r->riders, r->first, r->end, r->pipe);
}
