// Host check of csrc/gemm_plan.cpp (tests/test_gemm_plan_host.py compiles both with the address and undefined-behaviour sanitizers).
//   gemm_plan_check ROWS   ROWS: one descriptor per line, `name field=value ...`; a pointer field's value is 0 (absent) or 16 + the
//                          low four bits of its address
// Part 1 prints, for every row in both matrix arithmetics, the kernel the plan names as the kernel trace would show it, the reduce
// kernel behind it, the work items, the weight-gradient kernels' items per XCD, splitk and kchunk.  Part 2 plans 30 000 seeded
// random descriptors and checks what must hold for every one of them; the first violation is printed and the exit status is 1.
// It then prints the distinct (kernel, reduce kernel) pairs the sweep planned, one `pair: KERNEL | REDUCE` line each (a plan that
// sums by arrival counters as `counters/FALLBACK`), ahead of its summary line: the test requires a device-tested row for each.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <set>
#include <sstream>
#include <string>
#include <type_traits>

#include "gemm_plan.h"

namespace {

const as_gemm_env ENV[2] = {{AS_ARITH_FP32, 768, 8192}, {AS_ARITH_BF16X6, 768, 8192}};   // the MI355X: 256 CUs x 3 resident workgroups

const char* tf(bool b) { return b ? "true" : "false"; }

std::string kernel_name(const as_gemm_plan& p) {
    char s[128];
    switch (p.family) {
        case AS_GEMM_GENERAL:
            if (p.ext) snprintf(s, sizeof s, "gemm_f32_kernel<%d, %d, %s, %s, true, true>", p.tile_m, p.tile_n, tf(p.a_kc), tf(p.a_kc && p.b_kc));
            else snprintf(s, sizeof s, "gemm_f32_kernel<%d, %d, %s, %s, %s, false>", p.tile_m, p.tile_n, tf(p.a_kc), tf(p.b_kc), tf(p.fast));
            break;
        case AS_GEMM_S6: snprintf(s, sizeof s, "gemm_s6_kernel<%s, %s, %s>", tf(p.anc), tf(p.anc || p.bnc), tf(!p.anc && p.ext)); break;
        default: snprintf(s, sizeof s, "wgrad_f32_kernel<%d, %s, %s>", p.tile_n, tf(p.family == AS_GEMM_WGRAD_STREAMK), tf(p.split_arith));
    }
    return s;
}

std::string reduce_name(const as_gemm_plan& p, int kind) {
    switch (kind) {
        case AS_REDUCE_NONE: return "-";
        case AS_REDUCE_COUNTERS: return "counters/" + reduce_name(p, p.reduce_fallback);
        case AS_REDUCE_SPLITK: return "splitk_reduce_kernel";
        case AS_REDUCE_SPLITK4: return "splitk_reduce4_kernel";
        case AS_REDUCE_WGRAD: return "wgrad_reduce_kernel";
        default: return p.tile_n == 256 ? "wgrad_reduce_sk_kernel<256>" : "wgrad_reduce_sk_kernel<128>";
    }
}

// every field of a plan, for comparing two plans
std::string dump(const as_gemm_plan& p) {
    char s[512];
    snprintf(s, sizeof s, "%d %d %d %d%d%d%d%d%d%d%d%d%d%d %d %d %d %d %d %d %d %d %d %d %ld %ld", p.family, p.tile_m, p.tile_n, p.a_kc,
             p.b_kc, p.anc, p.bnc, p.fast, p.ext, p.split_arith, p.a_vec, p.b_vec, p.c_vec, p.vec_epi, p.k_tri, p.splitk, p.kchunk, p.reduce,
             p.reduce_fallback, p.xcd_panels, p.xcd_chunks, p.xcd_group, p.nkt, p.per_xcd, p.unit_per_wg, p.work);
    return s;
}

template <typename T>
T* fake(int slot, long bits) {   // a pointer that is never dereferenced: null, or a distinct address with the wanted low bits
    return bits ? reinterpret_cast<T*>(uintptr_t(0x100000000) * (slot + 1) + (bits & 15)) : nullptr;
}

bool set_field(as_gemm& g, const std::string& k, long v) {
#define I(f) if (k == #f) { g.f = (decltype(g.f))v; return true; }
#define P(f, slot) if (k == #f) { g.f = fake<typename std::remove_pointer<decltype(g.f)>::type>(slot, v); return true; }
    I(M) I(N) I(K) I(a_i) I(a_k) I(b_j) I(b_k) I(ldc) I(batch) I(a_batch) I(b_batch) I(c_batch) I(bias_batch) I(act) I(accumulate)
    I(b_kshift) I(b_kT) I(splitk_ws_floats) I(colsum_batch) I(precision) I(b_kshift_batch) I(cu_budget) I(res_ld) I(res_batch)
    I(mask_batch) I(relu_bits_batch) I(k_seg) I(k_tri)
    P(A, 0) P(B, 1) P(C, 2) P(bias, 3) P(splitk_ws, 4) P(colsum, 5) P(a_off, 6) P(b_off, 7) P(c_off, 8) P(bias_off, 9) P(res, 10)
    P(res_off, 11) P(mask_bits, 12) P(relu_bits, 13) P(a_seg_off, 14) P(b_seg_off, 15)
#undef I
#undef P
    return false;
}

int table(const char* path) {
    std::ifstream in(path);
    if (!in) { fprintf(stderr, "cannot read %s\n", path); return 1; }
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string name, kv;
        if (!(ss >> name)) continue;
        as_gemm g{};
        while (ss >> kv) {
            const size_t eq = kv.find('=');
            if (eq == std::string::npos || !set_field(g, kv.substr(0, eq), atol(kv.c_str() + eq + 1))) { fprintf(stderr, "bad field %s\n", kv.c_str()); return 1; }
        }
        for (int arith = 0; arith < 2; ++arith) {
            as_gemm_plan p;
            char err[512] = "";
            const int rc = as_gemm_plan_make(&g, &ENV[arith], &p, err, sizeof err);
            if (rc != 0) { printf("%s arith=%d refused (%d)\n", name.c_str(), arith, rc); continue; }
            printf("%s arith=%d %s reduce=%s work=%ld per_xcd=%d splitk=%d kchunk=%d\n", name.c_str(), arith, kernel_name(p).c_str(),
                   reduce_name(p, p.reduce).c_str(), p.work, p.per_xcd, p.splitk, p.kchunk);
        }
    }
    return 0;
}

struct Rng {
    uint64_t s;
    uint64_t next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
    long below(long n) { return (long)(next() % (uint64_t)n); }
    bool chance(int percent) { return below(100) < percent; }
};

int size(Rng& r) {   // 1 .. 7000, with the multiples the kernels care about well represented
    long v = r.chance(40) ? 1 + r.below(300) : 1 + r.below(7000);
    if (r.chance(50)) v = (v + 31) / 32 * 32;
    else if (r.chance(50)) v = (v + 3) / 4 * 4;
    return (int)(v > 7000 ? 7000 : v);
}
long stride(Rng& r, long least) {   // >= least: tight, padded to a multiple of 4, odd, or huge
    switch (r.below(6)) {
        case 0: return least;
        case 1: case 2: return (least + 3) / 4 * 4 + 4 * r.below(64);
        case 3: return least + 1 + r.below(7);
        case 4: return (least + 3) / 4 * 4;
        default: return least + (1L << (20 + r.below(21)));
    }
}

#define CHECK(cond)                                                                                      \
    do {                                                                                                 \
        if (!(cond)) {                                                                                   \
            printf("descriptor %d (arith %d): violated: %s\n  plan: %s\n", i, arith, #cond, dump(p).c_str()); \
            return 1;                                                                                    \
        }                                                                                                \
    } while (0)

int sweep() {
    Rng r{0x9E3779B97F4A7C15ull};
    long plans = 0, errors = 0, by_family[4] = {}, by_reduce[6] = {};
    std::set<std::string> pairs;
    for (int i = 0; i < 30000; ++i) {   // a third of the draws ask for a precision that is refused
        as_gemm g{};
        const bool wshape = r.chance(35), fwd = !wshape && r.chance(50);
        g.M = size(r); g.N = size(r); g.K = size(r);
        g.batch = r.chance(30) ? 1 : r.chance(90) ? 1 + (int)r.below(300) : 1 + (int)r.below(7000);
        const bool longk = r.chance(25);   // a long reduction over few tiles with a workspace: the split-K rules
        if (longk) { g.K = 32 * (8 + (int)r.below(211)); g.M = 4 * (1 + (int)r.below(200)); g.N = 4 * (1 + (int)r.below(200)); g.batch = 1 + (int)r.below(r.chance(50) ? 4 : 40); }
        if (r.chance(3)) (r.chance(50) ? g.M : g.batch) = (int)r.below(2) - 1;   // a non-positive size
        const int nseg = r.chance(12) ? 1 + (int)r.below(6) : 0;
        if (nseg) { g.k_seg = r.chance(90) ? 32 * (1 + (int)r.below(8)) : size(r); g.K = g.k_seg * nseg; }
        if (wshape || (!fwd && r.chance(10))) { g.a_i = 1; g.a_k = stride(r, g.M); } else { g.a_k = 1; g.a_i = stride(r, g.K); }
        if (wshape || !fwd) { g.b_j = 1; g.b_k = stride(r, g.N); } else { g.b_k = 1; g.b_j = stride(r, g.K); }
        if (r.chance(2)) g.a_k = g.a_i = 1 + r.below(2) * 7;   // both 1, or neither
        if (r.chance(2)) g.b_k = g.b_j = 1 + r.below(2) * 7;
        g.ldc = stride(r, g.N);
        const int odd = r.chance(85) ? 0 : 4 * (1 + (int)r.below(3));   // bytes off a 16-byte boundary
        g.A = fake<const float>(0, 16 + (r.chance(92) ? 0 : odd + 4));
        g.B = fake<const float>(1, 16 + (r.chance(92) ? 0 : 8));
        g.C = r.chance(99) ? fake<float>(2, 16 + (r.chance(90) ? 0 : 4)) : nullptr;
        auto bstride = [&](long least) { return r.chance(15) ? 0 : r.chance(85) ? (least + 3) / 4 * 4 : least + 1 + r.below(3); };
        g.a_batch = bstride((long)g.M * g.K); g.b_batch = bstride((long)g.N * g.K); g.c_batch = bstride((long)g.M * g.ldc);
        if (r.chance(40)) { g.bias = fake<const float>(3, 16 + (r.chance(90) ? 0 : 4)); g.bias_batch = bstride(g.N); }
        g.act = r.chance(55) ? 0 : (int)r.below(4) + (r.chance(2) ? 3 : 0);
        g.accumulate = r.chance(12);
        g.precision = r.chance(35) ? 3 : (int)r.below(4) + (r.chance(2) ? 3 : 0);
        if (wshape && r.chance(12)) { g.b_kT = 1 + (int)r.below(400); g.b_kshift = (int)r.below(3) - 1; g.b_kshift_batch = (int)r.below(3); }
        if (r.chance(wshape ? 70 : 25)) {
            g.splitk_ws = fake<float>(4, 16);
            g.splitk_ws_floats = r.chance(20) ? r.below(4096) : r.chance(50) ? r.below(1L << 22) : (20L << 20) + r.below(1L << 27);
        } else if (r.chance(5)) {
            g.splitk_ws_floats = 1L << 24;   // a size without a workspace
        }
        if (r.chance(wshape ? 50 : 8)) { g.colsum = fake<float>(5, 16); g.colsum_batch = bstride(g.M); }
        if (r.chance(25)) g.a_off = fake<const int64_t>(6, 16);
        if (r.chance(25)) g.b_off = fake<const int64_t>(7, 16);
        if (r.chance(25)) g.c_off = fake<const int64_t>(8, 16);
        if (r.chance(8)) g.bias_off = fake<const int64_t>(9, 16);
        if (r.chance(wshape ? 6 : 25)) { g.res = fake<const float>(10, 16 + (r.chance(90) ? 0 : 8)); g.res_ld = stride(r, g.N); g.res_batch = bstride((long)g.M * g.res_ld); }
        if (g.res && r.chance(40)) g.res_off = fake<const int64_t>(11, 16);
        if (r.chance(wshape ? 4 : 15)) { g.mask_bits = fake<const uint32_t>(12, 16); g.mask_batch = (long)g.M * ((g.N + 31) / 32); }
        if (r.chance(wshape ? 4 : 15)) { g.relu_bits = fake<uint32_t>(13, 16); g.relu_bits_batch = (long)g.M * ((g.N + 31) / 32); if (r.chance(80)) g.act = 1; }
        if (nseg && r.chance(95)) { g.a_seg_off = fake<const int64_t>(14, 16); g.b_seg_off = fake<const int64_t>(15, 16); }
        g.k_tri = r.chance(85) ? 0 : (int)r.below(3) + (r.chance(3) ? 2 : 0);
        if (longk && r.chance(80)) {
            g.bias = nullptr; g.act = 0; g.a_off = g.b_off = g.c_off = g.bias_off = nullptr; g.b_kT = 0;
            g.splitk_ws = fake<float>(4, 16);
            g.splitk_ws_floats = r.chance(15) ? r.below(1L << 20) : (8L << 20) + r.below(1L << 26);
        }
        g.cu_budget = r.chance(70) ? 0 : (int)r.below(513);
        const bool epi = g.res || g.mask_bits || g.relu_bits || g.k_seg;
        for (int arith = 0; arith < 2; ++arith) {
            as_gemm_plan p{};
            p.family = -1;
            char err[512] = "";
            const int rc = as_gemm_plan_make(&g, &ENV[arith], &p, err, sizeof err);
            if (g.precision != 0 && g.precision != 3) CHECK(rc == AS_ERR_BAD_ARG);   // 1 and 2 (once the on-the-fly split kernels) included
            if (rc != 0) {   // exactly one of an error or a plan
                CHECK(rc == AS_ERR_BAD_ARG && err[0] != 0 && strncmp(err, "as_gemm_f32: ", 13) == 0 && p.family == -1);
                ++errors;
                continue;
            }
            CHECK(err[0] == 0 && p.family >= AS_GEMM_GENERAL && p.family <= AS_GEMM_WGRAD_STREAMK);
            as_gemm_plan q;
            char err2[512] = "";
            CHECK(as_gemm_plan_make(&g, &ENV[arith], &q, err2, sizeof err2) == 0 && dump(p) == dump(q));   // planning is a pure function
            ++plans; ++by_family[p.family]; ++by_reduce[p.reduce];
            pairs.insert(kernel_name(p) + " | " + reduce_name(p, p.reduce));
            // the fp32 arithmetic never runs the library's split arithmetic
            if (arith == AS_ARITH_FP32) CHECK(p.family != AS_GEMM_S6 && !p.split_arith);
            CHECK(p.family != AS_GEMM_S6 || g.precision == 3);
            const bool wgrad = p.family == AS_GEMM_WGRAD || p.family == AS_GEMM_WGRAD_STREAMK;
            const int ktile = wgrad ? AS_WGRAD_BK : AS_GEMM_BK;
            CHECK(p.splitk >= 1 && (g.splitk_ws || (p.splitk == 1 && p.family != AS_GEMM_WGRAD_STREAMK)));
            CHECK(p.kchunk >= 1 && (long)(g.K + p.kchunk - 1) / p.kchunk == p.splitk);
            CHECK(p.splitk == 1 ? p.kchunk == g.K : p.kchunk % ktile == 0);
            CHECK((p.reduce == AS_REDUCE_NONE) == (p.splitk == 1 && p.family != AS_GEMM_WGRAD_STREAMK));
            CHECK(p.reduce != AS_REDUCE_COUNTERS || p.reduce_fallback == AS_REDUCE_SPLITK || p.reduce_fallback == AS_REDUCE_SPLITK4);
            const long cs_rows = g.colsum ? 1 : 0;
            if (p.splitk > 1 && !wgrad) CHECK(p.family == AS_GEMM_GENERAL && (long)p.splitk * g.batch * g.M * (g.N + cs_rows) <= g.splitk_ws_floats);
            if (p.splitk > 1 && wgrad) CHECK((long)p.splitk * g.batch * g.M * (g.N + cs_rows) <= g.splitk_ws_floats);
            if (p.family == AS_GEMM_WGRAD_STREAMK) CHECK(p.work * 2 * AS_WGRAD_PIECE_FLOATS <= g.splitk_ws_floats && p.nkt * 32 == g.K);
            if (wgrad) CHECK(8L * p.per_xcd >= p.work && 8L * p.per_xcd < p.work + 8);
            CHECK(p.work >= 1 && p.work < (1L << 31));
            // the extended operands only where a kernel reads them
            if (epi) CHECK((p.family == AS_GEMM_GENERAL && p.ext && p.a_kc) || (p.family == AS_GEMM_S6 && !p.anc && (p.ext || !(g.res || g.mask_bits || g.k_seg))));
            if (g.colsum) CHECK(g.a_i == 1 && (p.family == AS_GEMM_GENERAL ? !p.a_kc : p.family == AS_GEMM_S6 ? p.anc : wgrad));
            if (p.family == AS_GEMM_GENERAL && p.ext) CHECK(p.tile_m == p.tile_n && (p.a_kc || !p.b_kc));
            if (p.k_tri) CHECK(p.family == AS_GEMM_GENERAL && p.ext && p.k_tri == g.k_tri);
        }
    }
    for (const std::string& pair : pairs) printf("pair: %s\n", pair.c_str());
    printf("sweep: %ld plans, %ld refusals; families %ld %ld %ld %ld; reduces %ld %ld %ld %ld %ld %ld\n", plans, errors, by_family[0], by_family[1],
           by_family[2], by_family[3], by_reduce[0], by_reduce[1], by_reduce[2], by_reduce[3], by_reduce[4], by_reduce[5]);
    for (long n : by_family) if (n < 20) { printf("sweep: a kernel family was planned fewer than 20 times\n"); return 1; }
    for (long n : by_reduce) if (n < 20) { printf("sweep: a reduce kind was planned fewer than 20 times\n"); return 1; }
    if (errors < 1000) { printf("sweep: fewer than 1000 refusals\n"); return 1; }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s ROWS\n", argv[0]); return 2; }
    if (table(argv[1]) != 0) return 1;
    return sweep();
}
