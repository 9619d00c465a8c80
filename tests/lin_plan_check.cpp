// Host check of csrc/lin_plan.cpp (tests/test_lin_plan_host.py compiles both with the address and undefined-behaviour sanitizers).
//   lin_plan_check ROWS   ROWS: one descriptor per line, `name call=as_lin_try|as_lin_plain_s6|as_lin_out_try field=value ...`; a
//                         pointer field's value is 0 (absent) or 16 + the low four bits of its address; ksplit= / wps= are
//                         as_lin_plain_s6's arguments, counter= whether the stream has an arrival counter (default 1)
// Part 1 prints, for every row in both matrix arithmetics and with each of the two switches off (env=<arith><short_k><row_epi>),
// the launch the plan names: kernel as a kernel trace shows it, grid, workgroup size, dynamic LDS and the plan's other fields.
// Part 2 plans 20 000 seeded random descriptors of each kind and checks what must hold for every one of them; the first
// violation is printed and the exit status is 1.
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <sstream>
#include <string>
#include <type_traits>
#include <vector>

#include "gemm_plan.h"
#include "lin_plan.h"

namespace {

std::string kernel_name(const as_lin_plan& p) {
    char s[96];
    switch (p.family) {
        case AS_LIN_F32: snprintf(s, sizeof s, "lin_f32_kernel<64, %s, %d>", p.b_kc ? "true" : "false", p.epi); break;
        case AS_LIN_S6: snprintf(s, sizeof s, "lin_s6_kernel<%d>", p.epi); break;
        case AS_LIN_LNF_SHARED: return "lin_s6_lnf_shared_kernel";
        case AS_LIN_LNB_SHORT: return "lin_s6_lnb_short_kernel";
        case AS_LIN_PLAIN: snprintf(s, sizeof s, "lin_s6_plain_kernel<%d, %d>", p.nw, p.wps); break;
        case AS_LIN_OUT: return "lin_out_kernel";
        case AS_LIN_OUT_S6: return "lin_out_s6_kernel";
        default: return "none";
    }
    return s;
}
int block_size(const as_lin_plan& p) { return p.family == AS_LIN_PLAIN ? p.nw * 64 : p.family == AS_LIN_OUT_S6 ? 256 : 512; }

// every field of a plan: the launch as the code before the planner logged it, and for comparing two plans
std::string dump(const as_lin_plan& p) {
    if (p.family == AS_LIN_NONE) return "declined";
    char s[512];
    snprintf(s, sizeof s, "kernel=%s grid=%ldx%d block=%d lds=%d planes=%d n_big=%d big_per_batch=%d big_per_batch_rows=%d small_per_batch=%d groups=%d "
             "kchunk=%d row_epi=%d sums_loss=%d partials=%d", kernel_name(p).c_str(), p.tiles, p.ksplit, block_size(p), p.lds, p.planes, p.n_big,
             p.big_per_batch, p.big_per_batch_rows, p.small_per_batch, p.groups, p.kchunk, p.row_epi, p.sums_loss, p.partials);
    return s;
}

template <typename T>
T* fake(int slot, long bits, long base = 0x100000000) {   // never dereferenced: null, or a distinct address with the wanted low bits
    return bits ? reinterpret_cast<T*>(uintptr_t(base) * (slot + 1) + (bits & 15)) : nullptr;
}

#define I(f) if (k == #f) { g.f = (decltype(g.f))v; return true; }
#define P(f, slot) if (k == #f) { g.f = fake<typename std::remove_pointer<decltype(g.f)>::type>(slot, v); return true; }
bool set_field(as_lin& g, const std::string& k, long v) {
    I(lda) I(a_batch) I(ldb) I(b_batch) I(b_kc) I(bp_plane) I(bp_batch) I(bp_rows) I(ldc) I(c_batch) I(bias_batch) I(M) I(N) I(K) I(ka_valid)
    I(batch) I(act) I(epi) I(ldx) I(x_batch)
    P(A, 0) P(B, 1) P(Bp, 2) P(C, 3) P(bias, 4) P(rstd, 5) P(bits, 6) P(xhat, 7) P(rstd_in, 8) P(bits_in, 9)
    return false;
}
bool set_field(as_lin_out& g, const std::string& k, long v) {
    I(lda) I(a_batch) I(ldb) I(b_batch) I(b_rows) I(bias_batch) I(ldo) I(o_batch) I(M) I(N) I(K) I(batch) I(tgt_T) I(T) I(partial_capacity)
    I(bp_plane) I(bp_batch) I(bp_rows)
    P(A, 0) P(B, 1) P(Bp, 2) P(out, 3) P(bias, 4) P(tgt, 5) P(lengths, 6) P(dout, 7) P(partial, 8) P(loss, 9)
    return false;
}
#undef I
#undef P

const int SWITCHES[3][2] = {{1, 1}, {0, 1}, {1, 0}};   // short_k, row_epi: both on, each off

int table(const char* path) {
    std::ifstream in(path);
    if (!in) { fprintf(stderr, "cannot read %s\n", path); return 1; }
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string name, kv, call;
        if (!(ss >> name)) continue;
        as_lin l{};
        as_lin_out o{};
        long ksplit = 1, wps = 4, counter = 1;
        while (ss >> kv) {
            const size_t eq = kv.find('=');
            if (eq == std::string::npos) { fprintf(stderr, "bad field %s\n", kv.c_str()); return 1; }
            const std::string k = kv.substr(0, eq);
            const long v = atol(kv.c_str() + eq + 1);
            if (k == "call") call = kv.substr(eq + 1);
            else if (k == "ksplit") ksplit = v;
            else if (k == "wps") wps = v;
            else if (k == "counter") counter = v;
            else if (!(call == "as_lin_out_try" ? set_field(o, k, v) : set_field(l, k, v))) { fprintf(stderr, "bad field %s\n", kv.c_str()); return 1; }
        }
        for (int arith = 1; arith >= 0; --arith)
            for (const auto& sw : SWITCHES) {
                const as_lin_env env{arith, sw[0] != 0, sw[1] != 0, counter != 0, AS_LIN_LDS_MI355X};
                as_lin_plan p;
                if (call == "as_lin_try") as_lin_plan_make(&l, &env, &p);
                else if (call == "as_lin_plain_s6") as_lin_plain_plan_make(&l, (int)ksplit, (int)wps, &env, &p);
                else if (call == "as_lin_out_try") as_lin_out_plan_make(&o, &env, &p);
                else { fprintf(stderr, "bad call %s\n", call.c_str()); return 1; }
                printf("%s env=%d%d%d %s\n", name.c_str(), arith, sw[0], sw[1], dump(p).c_str());
            }
    }
    return 0;
}

struct Rng {
    uint64_t s;
    uint64_t next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
    long below(long n) { return (long)(next() % (uint64_t)n); }
    bool chance(int percent) { return below(100) < percent; }
    // a defect that makes the kernels decline: two descriptors in three are drawn without any, so that every family is planned often
    bool calm = false;
    bool flaw(int percent) { return chance(percent) && !calm; }
};

int rows(Rng& r) {   // M from 1 up: small, around the tile sizes, the benchmark's thousands, rarely huge
    if (r.flaw(4)) return r.chance(50) ? INT_MAX - (int)r.below(70) : (int)(1 + r.below(1L << 30));
    if (r.flaw(3)) return (int)r.below(2) - 1;   // 0, -1
    long v = r.chance(30) ? 1 + r.below(200) : r.chance(50) ? 1 + r.below(7000) : 1 + r.below(40000);
    if (r.chance(30)) v = (v + 31) / 32 * 32;
    return (int)v;
}
int heads(Rng& r) {
    if (r.flaw(4)) return r.chance(50) ? INT_MAX - (int)r.below(3) : (int)(1 + r.below(1L << 30));
    if (r.flaw(2)) return (int)r.below(2) - 1;
    if (r.chance(3)) return 1 + (int)r.below(1L << 23);   // (more heads than any model has; still a descriptor)
    return r.chance(25) ? 1 : r.chance(85) ? 1 + (int)r.below(16) : 1 + (int)r.below(3000);
}
int depth(Rng& r) {   // K on both sides of 128, mostly whole k-tiles
    long v = r.chance(60) ? 32 * (1 + r.below(8)) : !r.flaw(30) ? 16 * (1 + r.below(200)) : 1 + r.below(3000);
    if (r.flaw(2)) v = r.below(3) * 16 - 16;
    return (int)v;
}
long ld(Rng& r, long least) {   // >= least: tight, padded to a multiple of 4, odd, or huge (the kernels' 2^23 limit)
    switch (r.calm ? 2 + r.below(6) : r.below(8)) {
        case 0: return least + 1 + r.below(3);
        case 1: return least + (1L << (21 + r.below(6)));
        case 2: case 3: return (least + 3) / 4 * 4 + 4 * r.below(3000);
        default: return (least + 3) / 4 * 4;
    }
}
long bstride(Rng& r, long least) { return !r.flaw(12) ? (least + 3) / 4 * 4 : least + 1 + r.below(3); }
long ptr_bits(Rng& r, int absent_percent = 0) { return r.flaw(absent_percent) ? 0 : 16 + (!r.flaw(10) ? 0 : 4 * (1 + r.below(3))); }

template <typename L>
void planes(Rng& r, L& g, int slot) {
    if (r.chance(25)) return;
    g.Bp = fake<const uint16_t>(slot, 16 + (!r.flaw(7) ? 0 : 2 * (1 + r.below(7))));
    g.bp_rows = r.chance(45) ? 256 : r.chance(60) ? 128 : (int)r.below(400);
    g.bp_batch = (long)(g.K > 0 ? (g.K + 15) / 16 : 1) * (g.bp_rows > 0 ? g.bp_rows : 1) * 16 + (!r.flaw(6) ? 0 : 1 + r.below(7));
    g.bp_plane = (long)(g.batch > 0 ? g.batch : 1) * g.bp_batch + (!r.flaw(6) ? 0 : 1 + r.below(7));
}

as_lin random_lin(Rng& r) {
    as_lin g{};
    g.M = rows(r); g.batch = heads(r); g.K = depth(r);
    g.epi = r.chance(35) ? 0 : !r.flaw(3) ? 1 + (int)r.below(2) : 3;
    g.N = r.chance(g.epi ? 90 : 35) || (g.epi && r.calm) ? 256 : r.chance(30) ? 128 : !r.flaw(40) ? 4 * (1 + (int)r.below(70)) : (int)r.below(300);
    g.b_kc = g.epi == 1 ? !r.flaw(4) : g.epi == 2 ? r.flaw(4) : r.chance(60);
    g.A = fake<const float>(0, ptr_bits(r)); g.B = fake<const float>(1, ptr_bits(r));
    g.lda = ld(r, (long)g.K * (r.chance(50) ? 1 : (g.batch > 0 && g.batch < 64 ? g.batch : 1)));
    g.a_batch = r.chance(35) ? 0 : bstride(r, g.K);
    g.ldb = ld(r, g.b_kc ? g.K : g.N); g.b_batch = bstride(r, (long)g.N * (g.K > 0 ? g.K : 1));
    planes(r, g, 2);
    g.C = fake<float>(3, ptr_bits(r, 3)); g.ldc = ld(r, g.N); g.c_batch = bstride(r, g.N);
    if (r.chance(50)) { g.bias = fake<const float>(4, ptr_bits(r)); g.bias_batch = g.N; }
    g.act = r.chance(60) ? 0 : 1 + (int)r.below(2);
    g.ka_valid = r.chance(60) ? 0 : !r.flaw(15) ? 4 * (int)r.below(1 + (g.K > 0 ? g.K : 1) / 4) : 1 + (int)r.below(g.K > 0 ? g.K : 1);
    g.rstd = fake<float>(5, ptr_bits(r, 4)); g.bits = fake<unsigned long long>(6, ptr_bits(r, 4));
    g.xhat = fake<const float>(7, ptr_bits(r, 4)); g.ldx = g.ldc; g.x_batch = g.c_batch;
    g.rstd_in = fake<const float>(8, ptr_bits(r, 4)); g.bits_in = fake<const unsigned long long>(9, ptr_bits(r, 4));
    return g;
}

as_lin_out random_lin_out(Rng& r) {
    as_lin_out g{};
    g.M = rows(r); g.batch = heads(r); g.K = depth(r);
    g.N = r.chance(60) ? 4 * (1 + (int)r.below(32)) : !r.flaw(50) ? 2 * (1 + (int)r.below(64)) : (int)r.below(140);
    g.A = fake<const float>(0, ptr_bits(r)); g.B = fake<const float>(1, ptr_bits(r));
    g.lda = ld(r, (long)g.K * (g.batch > 0 && g.batch < 64 ? g.batch : 1)); g.a_batch = bstride(r, g.K);
    g.ldb = ld(r, g.K); g.b_rows = !r.flaw(10) ? 128 : (int)r.below(160); g.b_batch = bstride(r, (long)g.b_rows * (g.K > 0 ? g.K : 1));
    planes(r, g, 2);
    if (r.chance(70)) { g.bias = fake<const float>(4, ptr_bits(r)); g.bias_batch = g.N; }
    g.out = fake<float>(3, ptr_bits(r));
    const bool heads_layout = !r.flaw(8);
    g.ldo = heads_layout ? (long)g.batch * g.N : ld(r, g.N); g.o_batch = heads_layout ? g.N : bstride(r, g.N);
    if (r.chance(65)) {
        g.tgt = fake<const float>(5, ptr_bits(r)); g.tgt_T = 1 + r.below(500); g.lengths = fake<const int>(6, ptr_bits(r, 3));
        g.T = !r.flaw(4) ? 1 + (int)r.below(500) : 0; g.scale = 0.5f;
        g.dout = fake<float>(7, ptr_bits(r, 3)); g.partial = fake<float>(8, ptr_bits(r, 3));
        g.partial_capacity = r.chance(15) ? r.below(64) : r.chance(80) ? 1024 + r.below(1L << 16) : (1L << 31) + r.below(1L << 20);   // tiny, usual, beyond every list
        if (r.chance(80)) g.loss = fake<float>(9, 16);
    }
    return g;
}

as_lin_env random_env(Rng& r, int arith) {
    return as_lin_env{arith, !r.chance(25), !r.chance(25), r.chance(70), r.chance(80) ? AS_LIN_LDS_MI355X : 48 * 1024 + 4096 * (int)r.below(16)};
}

// the same descriptor at other addresses with the same null-ness and low four bits
template <typename T> void move_ptr(T*& p) { if (p) p = reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(p) + 0x7770000); }
void move_ptrs(as_lin& g) { move_ptr(g.A); move_ptr(g.B); move_ptr(g.Bp); move_ptr(g.C); move_ptr(g.bias); move_ptr(g.rstd); move_ptr(g.bits); move_ptr(g.xhat); move_ptr(g.rstd_in); move_ptr(g.bits_in); }
void move_ptrs(as_lin_out& g) { move_ptr(g.A); move_ptr(g.B); move_ptr(g.Bp); move_ptr(g.out); move_ptr(g.bias); move_ptr(g.tgt); move_ptr(g.lengths); move_ptr(g.dout); move_ptr(g.partial); move_ptr(g.loss); }

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int g_i, g_arith;
const char* g_kind;
#define CHECK(cond)                                                                                                            \
    do {                                                                                                                       \
        if (!(cond)) {                                                                                                         \
            printf("%s descriptor %d (arith %d): violated: %s\n  plan: %s\n", g_kind, g_i, g_arith, #cond, dump(p).c_str());   \
            return false;                                                                                                      \
        }                                                                                                                      \
    } while (0)

// The tile list as tile_of (lin_f32.hip) decodes it, over `members` batch members (heads, or head groups) of M rows: every row of
// every member in exactly one tile, every tile's first row below M, a total that fits a grid.
bool check_tiles(const as_lin_plan& p, int M, long members) {
    CHECK(p.tiles >= 1 && p.tiles <= INT_MAX && p.big_per_batch >= 1 && p.small_per_batch >= 1 && p.n_big >= 0);
    CHECK(p.big_per_batch_rows % 64 == 0 && p.big_per_batch_rows >= 0 && p.big_per_batch_rows <= M);
    const long n_small = p.tiles - p.n_big;
    if (p.tiles <= 8192) {   // tile by tile
        const int blocks = (M + 31) / 32;
        CHECK(members * blocks <= 4 * p.tiles);
        std::vector<unsigned char> seen((size_t)members * blocks, 0);
        for (long t = 0; t < p.tiles; ++t) {
            long bz, m0; int tm;
            if (t < p.n_big) { bz = t / p.big_per_batch; m0 = (t - bz * p.big_per_batch) * 64; tm = 2; }
            else { const long j = t - p.n_big; bz = j / p.small_per_batch; m0 = p.big_per_batch_rows + (j - bz * p.small_per_batch) * 32; tm = 1; }
            CHECK(bz >= 0 && bz < members && m0 >= 0 && m0 < M);
            for (int b = 0; b < tm && m0 + 32 * b < M; ++b) {
                CHECK(seen[(size_t)bz * blocks + m0 / 32 + b] == 0);
                seen[(size_t)bz * blocks + m0 / 32 + b] = 1;
            }
        }
        for (unsigned char s : seen) CHECK(s == 1);
    } else {                 // by counting: whole members of each kind of tile, the kinds meeting at big_per_batch_rows
        CHECK(p.n_big == (long)(p.big_per_batch_rows / 64) * members && (p.n_big == 0 || p.big_per_batch == p.big_per_batch_rows / 64));
        const int rest = M - p.big_per_batch_rows;
        CHECK(n_small == (long)((rest + 31) / 32) * members && (n_small == 0 || p.small_per_batch == (rest + 31) / 32));
    }
    return true;
}

bool planes_ok(const as_lin_env& env, const uint16_t* Bp, int K, long bp_plane, long bp_batch, long lda) {
    return env.arith == AS_ARITH_BF16X6 && K % 32 == 0 && Bp && aligned16(Bp) && bp_plane % 8 == 0 && bp_batch % 8 == 0 && lda < (1L << 23);
}

bool check_lin(const as_lin& g, const as_lin_env& env, const as_lin_plan& p) {
    if (p.family == AS_LIN_NONE) { CHECK(p.tiles == 0 && p.n_big == 0); return true; }
    CHECK(p.family == AS_LIN_F32 || p.family == AS_LIN_S6 || p.family == AS_LIN_LNF_SHARED || p.family == AS_LIN_LNB_SHORT);
    CHECK(g.M >= 1 && g.batch >= 1 && g.K >= 16 && g.K % 16 == 0 && g.N >= 4 && g.N <= 256 && aligned16(g.A) && aligned16(g.B));
    CHECK(p.planes == (p.family != AS_LIN_F32) && (!p.planes || (planes_ok(env, g.Bp, g.K, g.bp_plane, g.bp_batch, g.lda) && g.bp_rows >= 256)));
    CHECK(p.ksplit == 1 && p.kchunk == 0 && !p.row_epi && !p.sums_loss && p.partials == 0);
    CHECK(p.epi >= 0 && p.epi <= 2 && (p.epi != 1 || p.b_kc) && (p.epi != 2 || !p.b_kc) && (p.epi == 0 || (g.N == 256 && g.C)));
    const bool is_short = p.family == AS_LIN_LNF_SHARED || p.family == AS_LIN_LNB_SHORT;
    if (is_short) CHECK(g.K <= AS_LIN_SHORT_MAXK && env.short_k && p.epi == (p.family == AS_LIN_LNF_SHARED ? 1 : 2));
    if (p.family == AS_LIN_LNF_SHARED) {
        CHECK(g.a_batch == 0 && p.lds == g.K / 32 * 12 * 1024 + 32 * 1024 && p.lds <= env.lds_limit);
        // group t of `groups` takes heads [t * batch / groups, (t + 1) * batch / groups): every head in exactly one, none empty,
        // in the kernel's 32-bit arithmetic
        CHECK(p.groups >= 1 && p.groups <= g.batch && (long)p.groups * g.batch <= INT_MAX);
        return check_tiles(p, g.M, p.groups);
    }
    CHECK(p.groups == 0 && p.lds == 0);
    return check_tiles(p, g.M, g.batch);
}

bool check_plain(const as_lin& g, int ksplit, const as_lin_env& env, const as_lin_plan& p) {
    if (p.family == AS_LIN_NONE) { CHECK(p.tiles == 0 && p.n_big == 0); return true; }
    CHECK(p.family == AS_LIN_PLAIN && g.epi == 0 && g.M >= 1 && g.batch >= 1 && g.N >= 1 && g.N <= 256 && g.C && aligned16(g.A));
    CHECK(p.planes && planes_ok(env, g.Bp, g.K, g.bp_plane, g.bp_batch, g.lda) && g.bp_rows >= p.nw * 32 && g.N <= p.nw * 32);
    CHECK((p.nw == 4 || p.nw == 8) && (p.wps == 4 || (p.wps == 2 && p.nw == 4)));
    CHECK(p.kchunk >= 32 && p.kchunk % 32 == 0 && p.ksplit >= 1 && p.ksplit <= 65535);
    CHECK((long)(p.ksplit - 1) * p.kchunk < g.K && g.K <= (long)p.ksplit * p.kchunk);
    if (p.ksplit > 1) CHECK(!g.bias && !g.act);
    if (ksplit == AS_LIN_KSPLIT_AUTO) CHECK(p.ksplit <= 8 && (p.ksplit == 1 || p.tiles * p.ksplit <= 2 * AS_LIN_SLOTS));
    else CHECK(p.ksplit <= (ksplit < 1 ? 1 : ksplit));
    CHECK(p.groups == 0 && p.lds == 0 && !p.row_epi && !p.sums_loss && p.partials == 0);
    return check_tiles(p, g.M, g.batch);
}

bool check_out(const as_lin_out& g, const as_lin_env& env, const as_lin_plan& p) {
    if (p.family == AS_LIN_NONE) { CHECK(p.tiles == 0 && p.n_big == 0 && p.partials == 0); return true; }
    CHECK(p.family == AS_LIN_OUT || p.family == AS_LIN_OUT_S6);
    CHECK(g.M >= 1 && g.batch >= 1 && g.K >= 16 && g.K % 16 == 0 && g.N >= 4 && g.N <= 128 && g.N % 2 == 0 && g.b_rows >= g.N);
    CHECK(p.planes == (p.family == AS_LIN_OUT_S6) && (!p.planes || (planes_ok(env, g.Bp, g.K, g.bp_plane, g.bp_batch, g.lda) && g.bp_rows >= 128)));
    if (g.tgt) CHECK(p.tiles <= g.partial_capacity && g.lengths && g.dout && g.partial && g.T >= 1);
    CHECK(!p.row_epi || (g.tgt && env.row_epi && g.N % 4 == 0 && aligned16(g.out) && aligned16(g.dout) && aligned16(g.tgt)));
    CHECK(!p.sums_loss || (g.tgt && g.loss && env.counter));
    CHECK((p.partials == 0) == p.sums_loss && (p.sums_loss || p.partials == p.tiles));
    CHECK(p.ksplit == 1 && p.kchunk == 0 && p.groups == 0 && p.lds == 0);
    return check_tiles(p, g.M, g.batch);
}

#define PURE(same)                                                                                                                     \
    do {                                                                                                                               \
        if (!(same)) {                                                                                                                 \
            printf("%s descriptor %d (arith %d): the plan depends on more than fields, null-ness, low address bits and environment\n"  \
                   "  plan: %s\n  elsewhere: %s\n", g_kind, g_i, g_arith, dump(p).c_str(), dump(q).c_str());                           \
            return 1;                                                                                                                  \
        }                                                                                                                              \
    } while (0)

int sweep() {
    Rng r{0x9E3779B97F4A7C15ull};
    long by_family[8] = {}, shared_groups = 0, mixed_lists = 0, split = 0;
    for (g_i = 0; g_i < 20000; ++g_i) {
        r.calm = r.chance(67);
        as_lin l = random_lin(r);
        if (r.chance(2)) { l.M = 1 + (int)r.below(128); l.batch = 1 + (int)r.below(1L << 23); }   // few rows under very many heads
        as_lin pl = random_lin(r);   // the plain kernel's callers: epi 0, one plane image of 128 or 256 rows
        if (r.chance(90)) { pl.epi = 0; if (r.chance(80)) pl.act = 0, pl.bias = nullptr; }
        const int ksplit = r.chance(35) ? AS_LIN_KSPLIT_AUTO : r.chance(40) ? 1 : r.chance(90) ? 2 + (int)r.below(15) : (int)r.below(1L << 20) - 5;
        const int wps = r.chance(50) ? 2 : 4;
        const as_lin_out o = random_lin_out(r);
        for (g_arith = 0; g_arith < 2; ++g_arith) {
            const as_lin_env env = random_env(r, g_arith);
            as_lin_plan p, q;
            auto same_elsewhere = [&](auto g, auto&& make) {   // a pure function of fields, null-ness, low address bits and env
                move_ptrs(g);
                memset(&q, 0x5a, sizeof q);
                make(g, &q);
                return dump(p) == dump(q) && p.family == q.family && p.tiles == q.tiles && p.b_kc == q.b_kc && p.epi == q.epi && p.nw == q.nw && p.wps == q.wps;
            };
            g_kind = "as_lin";
            as_lin_plan_make(&l, &env, &p);
            if (!check_lin(l, env, p)) return 1;
            PURE(same_elsewhere(l, [&](const as_lin& g, as_lin_plan* out) { as_lin_plan_make(&g, &env, out); }));
            ++by_family[p.family];
            shared_groups += p.family == AS_LIN_LNF_SHARED && p.groups > 1 && p.groups < l.batch;
            mixed_lists += p.family != AS_LIN_NONE && p.n_big > 0 && p.tiles > p.n_big;
            g_kind = "as_lin (plain)";
            as_lin_plain_plan_make(&pl, ksplit, wps, &env, &p);
            if (!check_plain(pl, ksplit, env, p)) return 1;
            PURE(same_elsewhere(pl, [&](const as_lin& g, as_lin_plan* out) { as_lin_plain_plan_make(&g, ksplit, wps, &env, out); }));
            ++by_family[p.family];
            split += p.family == AS_LIN_PLAIN && p.ksplit > 1;
            g_kind = "as_lin_out";
            as_lin_out_plan_make(&o, &env, &p);
            if (!check_out(o, env, p)) return 1;
            PURE(same_elsewhere(o, [&](const as_lin_out& g, as_lin_plan* out) { as_lin_out_plan_make(&g, &env, out); }));
            ++by_family[p.family];
        }
    }
    printf("sweep: 120000 plans; families %ld %ld %ld %ld %ld %ld %ld %ld; %ld shared launches with several heads per group, %ld lists of both tile sizes, "
           "%ld split reductions\n", by_family[0], by_family[1], by_family[2], by_family[3], by_family[4], by_family[5], by_family[6], by_family[7],
           shared_groups, mixed_lists, split);
    for (long n : by_family) if (n < 100) { printf("sweep: a kernel family was planned fewer than 100 times\n"); return 1; }
    if (shared_groups < 20 || mixed_lists < 100 || split < 100) { printf("sweep: a rule was exercised too rarely\n"); return 1; }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s ROWS\n", argv[0]); return 2; }
    if (table(argv[1]) != 0) return 1;
    return sweep();
}
