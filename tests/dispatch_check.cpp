// The dispatch helpers of csrc/as_common.h (as_up_to, as_exactly, as_flag) on the host, for every list a call site uses and
// every v from 0 to two past the list's last entry: the N the functor receives is the one the if-ladder or switch that the
// helper replaced chose (written out below as plain ifs), the functor is called exactly once, and its result comes back.
// Row widths are also walked by D, through as_cdiv(D, 64), against the ladders over D.  tests/test_dispatch_host.py builds and
// runs this file, plainly and with the address and undefined-behaviour sanitizers.  Prints "dispatch: <n> checks" and exits 0,
// or one line per failure and exits 1.
#define AS_HOST_ONLY
#include "as_common.h"

static int g_checks = 0, g_failures = 0;

static void expect(bool ok, const char* what, int v, int got, int want, int calls) {
    ++g_checks;
    if (ok) return;
    ++g_failures;
    printf("FAIL %s: v=%d got N=%d want N=%d calls=%d\n", what, v, got, want, calls);
}

// ---- the ladders the helpers replaced, as they stood
static int norm_fwd_by_d(int D) { if (D <= 64) return 1; else if (D <= 128) return 2; else if (D <= 256) return 4; else return 8; }
static int norm_bwd_by_d(int D) { if (D <= 128) return 2; else if (D <= 256) return 4; else if (D <= 64 * 8) return 8; else return 44; }
static int ln_fwd_by_d(int D) {
    if (D <= 64) return 1; else if (D <= 128) return 2; else if (D <= 256) return 4; else if (D <= 512) return 8;
    else if (D <= 1024) return 16; else return 44;
}
static int softmax_by_tk(int Tk) {
    if (Tk <= 64) return 1; else if (Tk <= 128) return 2; else if (Tk <= 256) return 4; else if (Tk <= 512) return 8; else return 16;
}
static int norm_fwd(int c) { if (c <= 1) return 1; else if (c <= 2) return 2; else if (c <= 4) return 4; else return 8; }
static int norm_bwd(int c) { if (c <= 2) return 2; else if (c <= 4) return 4; else if (c <= 8) return 8; else return 44; }
static int ln_fwd(int c) {
    if (c <= 1) return 1; else if (c <= 2) return 2; else if (c <= 4) return 4; else if (c <= 8) return 8; else if (c <= 16) return 16;
    else return 44;
}
static int softmax(int c) { if (c <= 1) return 1; else if (c <= 2) return 2; else if (c <= 4) return 4; else if (c <= 8) return 8; else return 16; }
static int attn_nb(int nb) {
    if (nb <= 1) return 1;
    if (nb <= 2) return 2;
    if (nb <= 4) return 4;
    if (nb <= 6) return 6;
    if (nb <= 7) return 7;
    return 8;
}
static int edit_chunks(int c) {
    if (c <= 1) return 1; else if (c <= 2) return 2; else if (c <= 4) return 4; else if (c <= 8) return 8; else if (c <= 16) return 16;
    else return 32;
}
static int stem_bwd(int cin) { switch (cin) { case 1: return 1; case 2: return 2; case 3: return 3; default: return 4; } }
// exact matches: the N, or -1 where the parent took its other path
static int resident(int H) { switch (H) { case 32: return 32; case 64: return 64; case 128: return 128; default: return -1; } }
static int head_width(int dh) { if (dh == 64) return 64; else if (dh == 32) return 32; else if (dh == 16) return 16; return -1; }
static int stem_fwd(int cin) { switch (cin) { case 1: return 1; case 2: return 2; case 3: return 3; default: return -1; } }
static int three_way(int m) { return m == 0 ? 0 : (m == 1 ? 1 : (m == 2 ? 2 : -1)); }

template <int... Ns, typename L>
static void check_up_to(const char* what, int from, int to, L ladder) {
    for (int v = from; v <= to; ++v) {
        int calls = 0, got = -1;
        const int r = as_up_to<Ns...>(v, [&](auto n) { ++calls; got = decltype(n)::value; return 1000 + decltype(n)::value; });
        expect(calls == 1 && got == ladder(v) && r == 1000 + got, what, v, got, ladder(v), calls);
        calls = 0, got = -1;   // a functor that returns nothing, as the launching lambdas do
        as_up_to<Ns...>(v, [&](auto n) { ++calls; got = decltype(n)::value; });
        expect(calls == 1 && got == ladder(v), what, v, got, ladder(v), calls);
    }
}
template <int... Ns>
static int last_of() { constexpr int list[] = {Ns...}; return list[sizeof...(Ns) - 1]; }
template <int... Ns, typename L>
static void check_up_to(const char* what, L ladder) { check_up_to<Ns...>(what, 0, last_of<Ns...>() + 2, ladder); }

// the same through as_cdiv(D, unit), against a ladder over D itself
template <int... Ns, typename L>
static void check_up_to_cdiv(const char* what, int unit, L ladder_by_d) {
    for (int D = 1; D <= unit * (last_of<Ns...>() + 2); ++D) {
        int calls = 0, got = -1;
        as_up_to<Ns...>(as_cdiv(D, unit), [&](auto n) { ++calls; got = decltype(n)::value; });
        expect(calls == 1 && got == ladder_by_d(D), what, D, got, ladder_by_d(D), calls);
    }
}

template <int... Ns, typename L>
static void check_exactly(const char* what, int to, L table) {
    for (int v = 0; v <= to; ++v) {
        int calls = 0, got = -1, rc = -7;
        const bool hit = as_exactly<Ns...>(v, &rc, [&](auto n) { ++calls; got = decltype(n)::value; return 1000 + decltype(n)::value; });
        const int want = table(v);
        if (want < 0) expect(!hit && calls == 0 && rc == -7, what, v, got, want, calls);   // not in the list: not called, *rc untouched
        else expect(hit && calls == 1 && got == want && rc == 1000 + want, what, v, got, want, calls);
    }
}

int main() {
    check_up_to<1, 2, 4, 8>("normalize_fwd", norm_fwd);
    check_up_to<2, 4, 8, 44>("normalize_bwd", norm_bwd);
    check_up_to<1, 2, 4, 8, 16, 44>("layernorm_fwd", ln_fwd);
    check_up_to<1, 2, 4, 8, 16>("softmax", softmax);
    check_up_to<1, 2, 4, 6, 7, 8>("attention key blocks", attn_nb);
    check_up_to<1, 2, 4, 8, 16, 32>("edit distance chunks", edit_chunks);
    check_up_to<1, 2, 3, 4>("stem backward / weight gradient", 1, 6, stem_bwd);   // from 1: both entries refuse Cin < 1 before they dispatch
    check_up_to<7>("a list of one", [](int) { return 7; });

    check_up_to_cdiv<1, 2, 4, 8>("normalize_fwd by D", 64, norm_fwd_by_d);
    check_up_to_cdiv<2, 4, 8, 44>("normalize_bwd by D", 64, norm_bwd_by_d);
    check_up_to_cdiv<1, 2, 4, 8, 16, 44>("layernorm_fwd by D", 64, ln_fwd_by_d);
    check_up_to_cdiv<1, 2, 4, 8, 16>("softmax by Tk", 64, softmax_by_tk);
    check_up_to_cdiv<1, 2, 4, 6, 7, 8>("attention by Tk", 32, [](int Tk) { return attn_nb((Tk + 31) / 32); });

    check_exactly<32, 64, 128>("resident hidden size", 130, resident);
    check_exactly<64, 32, 16>("attention head width", 66, head_width);
    check_exactly<1, 2, 3>("stem forward", 5, stem_fwd);
    check_exactly<0, 1, 2>("three-way kernel choice", 4, three_way);

    for (int a = 0; a < 2; ++a) {
        int calls = 0, got = -1;
        const int r = as_flag(a != 0, [&](auto f) { ++calls; got = decltype(f)::value; return 1000 + decltype(f)::value; });
        expect(calls == 1 && got == a && r == 1000 + a, "flag", a, got, a, calls);
        calls = 0, got = -1;
        as_flag(a != 0, [&](auto f) { ++calls; got = decltype(f)::value; });
        expect(calls == 1 && got == a, "flag", a, got, a, calls);
        for (int b = 0; b < 2; ++b) {   // two flags, nested as the recurrences nest them
            calls = 0, got = -1;
            const int r2 = as_flag(a != 0, [&](auto fa) {
                return as_flag(b != 0, [&](auto fb) { ++calls; got = 2 * decltype(fa)::value + decltype(fb)::value; return 1000 + got; });
            });
            expect(calls == 1 && got == 2 * a + b && r2 == 1000 + got, "flag pair", 2 * a + b, got, 2 * a + b, calls);
        }
    }
    printf("dispatch: %d checks\n", g_checks);
    return g_failures ? 1 : 0;
}
