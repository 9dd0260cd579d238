// Stand-alone check of the thin Linear's host side (anemoi_models_amd/csrc/gemm_thin_plan.hpp): which argument blocks are
// taken, refused (ANEMOI_ERR_UNSUPPORTED) or rejected (ANEMOI_ERR_INVALID), and the launch geometry of those taken.  It calls
// no device function and needs no GPU; pointers are looked at for NULL and alignment only.  Build it with the host
// sanitizers and run it (tests/test_thin_plan_cpu.py does):
//
//   hipcc -x hip --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/thin_plan_check.cpp -o thin_plan_check && ./thin_plan_check
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../anemoi_models_amd/csrc/gemm_thin_plan.hpp"

using namespace anemoi;

static int failures = 0;

#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::printf("FAILED line %d: %s (%s)\n", __LINE__, #cond, err_buf()); \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

static anemoi_linear_thin_args base(int n, int k, int64_t m, char* mem) {
  anemoi_linear_thin_args a;
  std::memset(&a, 0, sizeof(a));
  a.struct_bytes = sizeof(a);
  a.out_dtype = ANEMOI_BF16;
  a.x = mem;
  a.w = mem + 64;
  a.y = mem + 128;
  a.ldx = k;
  a.ldy = n;
  a.M = m;
  a.N = n;
  a.K = k;
  return a;
}

int main() {
  char* mem = static_cast<char*>(std::aligned_alloc(64, 4096));
  thin::Plan p;
  const int cus = 256;

  // every shape of the table, every row count around a block: taken, and the grid never exceeds the work
  for (int i = 0; i < thin::N_SHAPES; ++i) {
    const thin::Shape& s = thin::SHAPES[i];
    for (int64_t m : {(int64_t)1, (int64_t)15, (int64_t)16, (int64_t)17, (int64_t)63, (int64_t)197, (int64_t)542080, (int64_t)1 << 34}) {
      for (int out : {ANEMOI_BF16, ANEMOI_F32}) {
        anemoi_linear_thin_args a = base(s.n, s.k, m, mem);
        a.out_dtype = out;
        std::memset(&p, 0xff, sizeof(p));
        EXPECT(thin::plan(&a, cus, p) == ANEMOI_OK);
        EXPECT(p.shape == i && p.row_blocks == (m + 15) / 16 && p.grid_y == 1);
        const int64_t items = s.mode == thin::MODE_ROWS ? (p.row_blocks + 3) / 4 : p.row_blocks;
        EXPECT(p.grid_x >= 1 && (int64_t)p.grid_x <= items && (int64_t)p.grid_x <= cus);
        // paired bf16 stores only where a wave holds an even number of tiles and a product is stored as bf16
        const int tiles = s.n / 16 / (s.mode == thin::MODE_NSPLIT ? 4 : 1);
        EXPECT(p.pair == (s.mode != thin::MODE_KSPLIT && tiles % 2 == 0 && out == ANEMOI_BF16));
        float stats_out[2];
        a.stats_out = stats_out;
        a.y = nullptr;  // statistics only: no product buffer needed
        EXPECT(thin::plan(&a, cus, p) == ANEMOI_OK && p.pair == 0);
        a.residual = mem + 256;
        a.ldr = s.n;
        EXPECT(thin::plan(&a, cus, p) == ANEMOI_ERR_UNSUPPORTED);  // statistics only with a residual
      }
    }
    // batched: the register-resident (K <= 256) shapes only, never with a fold or statistics
    anemoi_linear_thin_args a = base(s.n, s.k, 1000, mem);
    a.batch = 16;
    a.ldx = 16 * s.k;
    a.ldy = 16 * s.n;
    a.stride_x = s.k;
    a.stride_w = (int64_t)s.n * s.k;
    a.stride_y = s.n;
    const int rc = thin::plan(&a, cus, p);
    EXPECT(rc == (s.mode == thin::MODE_KSPLIT ? ANEMOI_ERR_UNSUPPORTED : ANEMOI_OK));
    if (rc == ANEMOI_OK) {
      EXPECT(p.grid_y == 16 && p.grid_x >= 1 && (int64_t)p.grid_x * 16 <= cus + 15);
      a.colsum = reinterpret_cast<const float*>(mem + 512);
      a.stats = reinterpret_cast<const float*>(mem + 1024);
      EXPECT(thin::plan(&a, cus, p) == ANEMOI_ERR_UNSUPPORTED);
      a.colsum = a.stats = nullptr;
      a.stride_x = s.k + 4;
      EXPECT(thin::plan(&a, cus, p) == ANEMOI_ERR_INVALID);
      a.stride_x = s.k;
      a.stride_y = s.n + 4;
      EXPECT(thin::plan(&a, cus, p) == ANEMOI_ERR_INVALID);
      a.stride_y = -8;
      EXPECT(thin::plan(&a, cus, p) == ANEMOI_ERR_INVALID);
    }
  }

  // shapes outside the table: refused, whatever else the block holds
  for (int n : {8, 16, 48, 64, 80, 128, 256, 512})
    for (int k : {32, 64, 128, 256, 512, 1024, 2048}) {
      bool in_table = false;
      for (int i = 0; i < thin::N_SHAPES; ++i) in_table |= thin::SHAPES[i].n == n && thin::SHAPES[i].k == k;
      anemoi_linear_thin_args a = base(n, k, 100, mem);
      EXPECT(thin::plan(&a, cus, p) == (in_table ? ANEMOI_OK : ANEMOI_ERR_UNSUPPORTED));
      a.x = nullptr;  // (the shape is judged first: a refusal says "not this kernel", not "bad call")
      EXPECT(thin::plan(&a, cus, p) == (in_table ? ANEMOI_ERR_INVALID : ANEMOI_ERR_UNSUPPORTED));
    }

  // the handshake and the plain argument errors
  {
    anemoi_linear_thin_args a = base(80, 1024, 100, mem);
    EXPECT(thin::plan(nullptr, cus, p) == ANEMOI_ERR_INVALID);
    a.struct_bytes -= 8;
    EXPECT(thin::plan(&a, cus, p) == ANEMOI_ERR_INVALID && std::strstr(err_buf(), "out of sync") != nullptr);
    a = base(80, 1024, 100, mem);
    a.out_dtype = 7;
    EXPECT(thin::plan(&a, cus, p) == ANEMOI_ERR_INVALID);
    a = base(80, 1024, 0, mem);
    EXPECT(thin::plan(&a, cus, p) == ANEMOI_ERR_UNSUPPORTED);
    a = base(80, 1024, -1, mem);
    EXPECT(thin::plan(&a, cus, p) == ANEMOI_ERR_INVALID);
    a = base(80, 1024, ((int64_t)1 << 34) + 1, mem);
    EXPECT(thin::plan(&a, cus, p) == ANEMOI_ERR_UNSUPPORTED);
    a = base(80, 1024, 100, mem);
    a.ldx = 1016;
    EXPECT(thin::plan(&a, cus, p) == ANEMOI_ERR_INVALID);  // below the row width
    a.ldx = 1028;
    EXPECT(thin::plan(&a, cus, p) == ANEMOI_ERR_INVALID);  // not a multiple of 8
    a.ldx = 1032;
    EXPECT(thin::plan(&a, cus, p) == ANEMOI_OK);
    a.x = mem + 2;
    EXPECT(thin::plan(&a, cus, p) == ANEMOI_ERR_INVALID);
    a.x = mem;
    a.ldy = 84;  // bf16: a multiple of 8; f32: of 4
    EXPECT(thin::plan(&a, cus, p) == ANEMOI_ERR_INVALID);
    a.out_dtype = ANEMOI_F32;
    EXPECT(thin::plan(&a, cus, p) == ANEMOI_OK);
    a.colsum = reinterpret_cast<const float*>(mem + 512);  // a fold needs both operands
    EXPECT(thin::plan(&a, cus, p) == ANEMOI_ERR_INVALID);
    a.stats = reinterpret_cast<const float*>(mem + 1024 + 4);
    EXPECT(thin::plan(&a, cus, p) == ANEMOI_ERR_INVALID);  // stats not 8-byte aligned
    a.stats = reinterpret_cast<const float*>(mem + 1024);
    EXPECT(thin::plan(&a, cus, p) == ANEMOI_OK);
    a.bias = reinterpret_cast<const float*>(mem + 2048 + 4);
    EXPECT(thin::plan(&a, cus, p) == ANEMOI_ERR_INVALID);
    a.bias = reinterpret_cast<const float*>(mem + 2048);
    a.residual = mem + 3072;
    a.ldr = 80;
    EXPECT(thin::plan(&a, cus, p) == ANEMOI_OK);
    a.ldr = 72;
    EXPECT(thin::plan(&a, cus, p) == ANEMOI_ERR_INVALID);
    a.ldr = 80;
    EXPECT(thin::plan(&a, 0, p) == ANEMOI_ERR_INVALID);  // no device
    for (int c : {1, 8, 80, 256, 304}) {
      EXPECT(thin::plan(&a, c, p) == ANEMOI_OK && (int)p.grid_x == (c < 7 ? c : 7));  // 100 rows = 7 row blocks
    }
  }
  std::free(mem);
  std::printf(failures == 0 ? "thin_plan_check: ok\n" : "thin_plan_check: %d FAILED\n", failures);
  return failures == 0 ? 0 : 1;
}
