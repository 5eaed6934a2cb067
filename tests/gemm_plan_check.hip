// Stand-alone driver of plan_gemm() (arcflow_amd/csrc/afx_gemm_plan.h) for tests/test_gemm_plan_cpu.py: batches with fake pointers, explicit settings,
// 256 CUs; one line per case.  No kernel and no HIP runtime call: runs without a GPU.
//   hipcc -std=c++17 -I arcflow_amd/csrc tests/gemm_plan_check.hip -o gemm_plan_check     (`gemm_plan_check time` prints the host cost of a plan instead)
#include <chrono>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "afx_gemm_plan.h"

using namespace afx;

template <typename T>
static T* fake() { return reinterpret_cast<T*>(uintptr_t(0x10000)); }

static GemmProblem prob(int M, int N, int K) {
  GemmProblem p{};
  p.A = fake<const uint16_t>(); p.W = fake<const uint16_t>(); p.C = fake<uint16_t>();
  p.lda = p.ldw = K; p.ldc = N;
  p.M = M; p.N = N; p.K = K;
  p.rows_per_batch = M > 0 ? M : 1;
  return p;
}
static GemmProblem f32(GemmProblem p, int out_f32, int split_k = 0) { p.out_f32 = out_f32; p.split_k = split_k; return p; }
static GemmProblem qk(GemmProblem p, int D) {
  p.qk_D = D; p.qk_wk = p.qk_wq = p.rope_cos = p.rope_sin = fake<const float>();
  p.rope_period = p.rope_rows = 4608;
  return p;
}
static GemmProblem conv(GemmProblem p) { p.conv_cin_tiles = p.K / (9 * 64); p.conv_wp = 34; p.conv_hp = 34; return p; }
static GemmProblem fp8(GemmProblem p) { p.fp8 = 1; p.a_scale = p.w_scale = fake<const float>(); return p; }
static GemmProblem mx(GemmProblem p) { p = fp8(p); p.a_mx = fake<const uint8_t>(); p.ld_mx = p.K / 128; return p; }
static GemmProblem c8(GemmProblem p, int epi) {
  p = fp8(p); p.c8 = fake<uint8_t>(); p.c_mx = fake<uint8_t>(); p.ldc8 = p.N; p.ld_cmx = p.N / 128; p.epi = epi;
  if (epi == EPI_GATE_RES) { p.gate = fake<const float>(); p.res = fake<const uint16_t>(); }
  return p;
}
static GemmProblem drop(GemmProblem p, bool gate) {
  p.epi = EPI_GATE_RES; p.res = fake<const uint16_t>(); p.ldr = p.N; p.drop_on = 1; p.drop_inv_keep = 1.0f;
  if (gate) p.gate = fake<const float>();
  return p;
}
static GemmBatch batch(std::initializer_list<GemmProblem> ps) {
  GemmBatch b{};
  for (const GemmProblem& p : ps) b.p[b.nprob++] = p;
  b.total_tiles = b.group_m = -1;
  return b;
}
static GemmMode mode(int impl = 3, int tile = 0) { GemmMode m; m.impl = impl; m.tile = tile; return m; }

static const char* kFamily[] = {"v3", "v3conv", "v3f8", "8phase"};

// name: ok <family>[+mx | +fp8] <tm>x<tn> total=<tiles> group_m=<g> persist=<p> grid=<work-groups> [tiles <tiles_m>x<tiles_n>*<split_k>@<tile_start> per problem]
static GemmPlan show(const char* name, GemmBatch b, const GemmMode& m, int cus = 256, bool problems = false) {
  const GemmPlan pl = plan_gemm(b, m, cus);
  if (pl.status != GemmPlan::OK) {
    printf("%s: %s\n", name, pl.status == GemmPlan::EMPTY ? "empty" : "invalid");
    return pl;
  }
  printf("%s: ok %s%s %dx%d total=%d group_m=%d persist=%d grid=%d", name, kFamily[pl.family],
         !pl.flag ? "" : pl.family == GemmPlan::V3_FP8 ? "+mx" : "+fp8", 32 * pl.mi, 32 * pl.nj, pl.total, b.group_m, pl.persist, pl.grid);
  if (b.total_tiles != pl.total) printf(" total_tiles=%d", b.total_tiles);      // (never: the batch carries the plan's count)
  if (problems)
    for (int i = 0; i < b.nprob; ++i) printf(" tiles %dx%d*%d@%d", b.p[i].tiles_m, b.p[i].tiles_n, b.p[i].split_k, b.p[i].tile_start);
  printf("\n");
  return pl;
}

int main(int argc, char** argv) {
  const GemmBatch flux3072 = batch({prob(4096, 3072, 3072), prob(512, 3072, 3072)});
  const GemmBatch flux_qkv = batch({qk(prob(4096, 9216, 3072), 3072), qk(prob(512, 9216, 3072), 3072)});
  const GemmBatch qwen_qkv = batch({qk(prob(4096, 9216, 3072), 3072), qk(prob(128, 9216, 3072), 3072)});
  const GemmBatch conv128 = batch({conv(prob(34 * 34, 128, 9 * 128))}), conv256 = batch({conv(prob(34 * 34, 256, 9 * 256))});
  if (argc > 1 && !strcmp(argv[1], "time")) {      // host cost of one plan (the cost-model path / the q-k path), ns per call
    for (const GemmBatch* src : {&flux3072, &flux_qkv}) {
      const int n = 2000000;
      long sink = 0;
      const GemmMode m = mode();
      const auto t0 = std::chrono::steady_clock::now();
      for (int i = 0; i < n; ++i) {
        GemmBatch b = *src;
        b.p[0].M += i & 1;
        sink += plan_gemm(b, m, 256).total;
      }
      const double ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count() / n;
      printf("plan_gemm (with the batch copy): %.1f ns per call (%ld)\n", ns, sink);
    }
    return 0;
  }
  // ---- bf16 tile choice, default settings
  show("flux_n3072", flux3072, mode(), 256, true);
  show("flux_n3072_f32", batch({f32(prob(4096, 3072, 3072), 1), f32(prob(512, 3072, 3072), 1)}), mode());
  show("flux_n12288", batch({prob(4096, 12288, 3072), prob(512, 12288, 3072)}), mode());
  show("lora_n256", batch({prob(4608, 256, 3072)}), mode());
  // ---- q / k fusion
  show("qk_qwen", qwen_qkv, mode());
  show("qk_flux", flux_qkv, mode());
  show("qk_flux_tile6", flux_qkv, mode(3, 6));
  show("qk_flux_tile2", flux_qkv, mode(3, 2));
  show("qk_qwen_impl2", qwen_qkv, mode(2, 0));
  show("qk_flux_impl2", flux_qkv, mode(2, 0));
  {
    GemmBatch b = flux_qkv;
    b.p[1].rope_sin = nullptr;
    show("qk_no_table", b, mode());
  }
  // ---- overrides
  for (int t = 1; t <= 6; ++t) {
    char name[32];
    snprintf(name, sizeof name, "tile%d", t);
    show(name, flux3072, mode(3, t));
  }
  show("tile5_f32", batch({f32(prob(4096, 3072, 3072), 1)}), mode(3, 5));
  {
    GemmMode m = mode();
    m.group_m = 9;
    show("group_m9", flux3072, m);
    show("group_m9_conv", conv128, m);
    show("group_m9_8phase", flux3072, [&] { GemmMode n = m; n.impl = 2; return n; }());
  }
  show("impl2", flux3072, mode(2, 0));
  // ---- not for the one-wave-per-SIMD kernel: the 8-phase kernel takes the launch
  {
    GemmBatch b = flux3072;
    b.p[0].pre = fake<const uint16_t>();
    show("pre", b, mode());
  }
  show("splitk4", batch({f32(prob(256, 3072, 4608), 3, 4)}), mode(), 256, true);
  show("splitk_ignored", batch({f32(prob(256, 3072, 4608), 0, 4)}), mode(), 256, true);      // split_k without slabs: normalised to 1
  show("k32", batch({prob(512, 512, 32)}), mode());
  show("f32_gelu", batch({[] { GemmProblem p = f32(prob(512, 512, 512), 1); p.epi = EPI_GELU; return p; }()}), mode());
  // ---- convolutions
  show("conv_n128", conv128, mode());
  show("conv_n256", conv256, mode());
  show("conv_tile1", conv128, mode(3, 1));
  show("conv_impl2", conv128, mode(2, 0));
  show("conv_mixed", batch({conv128.p[0], prob(1156, 128, 1152)}), mode());
  // ---- fp8
  show("fp8_120", batch({fp8(prob(2048, 3840, 3072))}), mode());
  show("fp8_128", batch({fp8(prob(2048, 4096, 3072))}), mode());
  show("fp8_qwen", batch({fp8(prob(4096, 3072, 3072)), fp8(prob(128, 3072, 3072))}), mode());
  for (int t = 1; t <= 2; ++t) {
    GemmMode m = mode();
    m.fp8_tile = t;
    show(t == 1 ? "fp8_tile1" : "fp8_tile2", batch({fp8(prob(4096, 3072, 3072)), fp8(prob(128, 3072, 3072))}), m);
  }
  {
    GemmMode m = mode();
    m.fp8_v3_min = 0;
    show("fp8_min0", batch({fp8(prob(512, 3072, 3072))}), m);
    m = mode();
    m.fp8_v3 = false;
    show("fp8_v3_off", batch({fp8(prob(4096, 3072, 3072))}), m);
    show("fp8_v3_off_mx", batch({mx(prob(4096, 3072, 3072))}), m);
  }
  show("fp8_impl2", batch({fp8(prob(4096, 3072, 3072))}), mode(2, 0));
  show("mx", batch({mx(prob(512, 3072, 3072))}), mode());
  show("mx_k3200", batch({mx(prob(512, 3072, 3200))}), mode());
  show("mx_mixed", batch({mx(prob(512, 3072, 3072)), fp8(prob(512, 3072, 3072))}), mode());
  show("c8_gelu", batch({c8(prob(512, 12288, 3072), EPI_GELU)}), mode());
  show("c8_gate_res", batch({c8(prob(512, 12288, 3072), EPI_GATE_RES)}), mode());
  show("c8_impl2", batch({c8(prob(512, 12288, 3072), EPI_GELU)}), mode(2, 0));
  show("fp8_qk", batch({qk(mx(prob(4096, 9216, 3072)), 3072), qk(mx(prob(128, 9216, 3072)), 3072)}), mode());
  // ---- other validation
  show("drop", batch({drop(prob(4608, 3072, 256), false)}), mode());
  show("drop_gate", batch({drop(prob(4608, 3072, 256), true)}), mode());
  show("drop_impl2", batch({drop(prob(4608, 3072, 256), false)}), mode(2, 0));
  show("drop_k32", batch({drop(prob(4608, 3072, 32), false)}), mode());
  {
    GemmProblem p = prob(3072, 4600, 3072);
    p.w_perm16 = 1;
    show("perm16_n4600", batch({p}), mode());
    p.N = p.ldc = 4608;
    show("perm16_n4608", batch({p}), mode());
    show("perm16_impl2", batch({p}), mode(2, 0));
  }
  show("empty", batch({prob(0, 3072, 3072)}), mode());
  show("empty_qk", batch({qk(prob(0, 9216, 3072), 3072)}), mode());
  show("empty_conv", batch({conv(prob(0, 128, 1152))}), mode());
  show("empty_8phase", batch({prob(0, 3072, 3072)}), mode(2, 0));
  // ---- the persistent walk: more tiles than resident work-groups, and a grid that is a multiple of the 8 XCDs
  for (int ps = 0; ps <= 3; ++ps) {
    GemmMode m = mode();
    m.persist = ps;
    char name[32];
    snprintf(name, sizeof name, "persist%d", ps);
    show(name, batch({prob(4096, 12288, 3072), prob(512, 12288, 3072)}), m);
  }
  {
    GemmMode m = mode();
    m.persist = 1;
    show("persist1_one_round", flux3072, m);
    show("persist1_cus250", batch({prob(4096, 12288, 3072), prob(512, 12288, 3072)}), m, 250);
    show("persist1_conv", batch({conv(prob(514 * 514, 128, 1152))}), m);
    show("persist1_fp8", batch({fp8(prob(4608, 12288, 3072))}), m);
    show("persist1_8phase", batch({prob(4608, 12288, 3072)}), [&] { GemmMode n = m; n.impl = 2; return n; }());
    m.tile = 4;
    show("persist1_128x128", batch({prob(4608, 3072, 3072)}), m);
    m.persist = 2;
    show("persist2_128x128_one_round", batch({prob(4608, 256, 3072)}), m);
  }
  // ---- the predicates callers ask first say what the planner does with a matching batch
  const int modes[3][2] = {{3, 0}, {3, 1}, {2, 0}};
  for (const auto& mt : modes) {
    const GemmMode m = mode(mt[0], mt[1]);
    GemmBatch b = flux_qkv;
    GemmPlan pl = plan_gemm(b, m, 256);
    printf("pred qk_fusion (%d,%d): available=%d planned=%d\n", mt[0], mt[1], (int)gemm_qk_fusion_available(m), (int)(pl.status == GemmPlan::OK && pl.family == GemmPlan::V3_BF16));
    b = batch({drop(prob(4608, 3072, 256), false)});
    pl = plan_gemm(b, m, 256);
    printf("pred dropres (%d,%d): available=%d planned=%d\n", mt[0], mt[1], (int)gemm_dropres_available(m), (int)(pl.status == GemmPlan::OK && pl.family == GemmPlan::V3_BF16));
    b = conv128;
    b.p[0].gn_stats = fake<double>(); b.p[0].gn_gs = 4; b.p[0].gn_groups = 32;
    pl = plan_gemm(b, m, 256);
    printf("pred conv_stats (%d,%d): available=%d planned=%d\n", mt[0], mt[1], (int)gemm_conv_stats_available(m), (int)(pl.status == GemmPlan::OK && pl.family == GemmPlan::V3_CONV));
    for (int K : {3072, 3200, 256}) {
      b = batch({mx(prob(512, 3072, K))});
      pl = plan_gemm(b, m, 256);
      printf("pred fp8_mx_ok (%d,%d) K=%d: available=%d planned=%d\n", mt[0], mt[1], K, (int)gemm_fp8_mx_ok(m, K),
             (int)(pl.status == GemmPlan::OK && pl.family == GemmPlan::V3_FP8 && pl.flag));
    }
  }
  {
    GemmMode m = mode();
    m.qk_fuse = false;      // the callers' switch (a separate kv_prep launch instead): the planner itself still takes a q / k batch
    printf("pred qk_fusion qk_fuse=0: available=%d\n", (int)gemm_qk_fusion_available(m));
    m.fp8_v3 = false;
    printf("pred fp8_mx_ok fp8_v3=0: available=%d\n", (int)gemm_fp8_mx_ok(m, 3072));
  }
  return 0;
}
