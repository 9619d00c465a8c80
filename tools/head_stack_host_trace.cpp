// Host-only trace of csrc/artspeech.hip: its object is linked against THIS file, in which every function it calls -- the
// library's launchers, as_gemm_f32, the profiler scopes and the HIP event / stream calls -- only prints its name and the bytes
// of its arguments (descriptors as their bytes, as_planes_job field for field since brace-initialised ones carry padding;
// pointers are the fake addresses main() hands in).  Streams and events print as S<n> / E<n>, n = their rank of first
// appearance in the entry-point call (S0: the caller's stream; as_opts.fold_wait_event, which the caller owns: Eext), so that
// the text depends neither on how many events the library creates nor on which of them two calls share.  Besides the calls there are "@slab <pointer> <stream>" behind every launch
// that is handed a split-K slab, "slot= <event>" / "slot> <event>" when the stop-event slot is armed / emptied by its owner,
// "@carry <event> <stream>" when a launch consumes it (mode 256), and the slot's content behind every entry point's result
// (tests/test_step_schedule_host.py reads these).  main() drives as_head_fwd /
// as_head_bwd / as_artspeech_fwd / as_artspeech_bwd / as_artspeech_dw2 over hidden sizes, output widths, head counts, row
// counts, option sets and overlap on / off, and forces each "1 = launched, 0 = not a case" callee to decline in turn (g_mode),
// so that every fallback is posed -- also those no legal as_dims reaches on the GPU (head.gemm2, headb.dx2).  Two commits
// enqueue the same work with the same arguments when their outputs are equal: no GPU needed.  `--small` runs every mode and option
// set at one geometry (H = 128, N = 50, 3 and 11 heads, 37 and 512 rows): what tests/test_step_schedule_host.py replays.
//   hipcc -O1 -std=c++17 -Iinclude -Iartspeech_amd/csrc -x hip --offload-arch=gfx950 -c tools/head_stack_host_trace.cpp -o trace.o
//   hipcc --offload-arch=gfx950 trace.o artspeech_amd/csrc/build/artspeech.o artspeech_amd/csrc/build/lin_plan.o -o head_stack_host_trace && ./head_stack_host_trace | sha256sum
// The heads' dx1 asks the planner (lin_plan.cpp, linked in as it is) how many slabs as_lin_plain_s6 will write.  With
// -DDX1_BEFORE_PLANNER (and without lin_plan.o) a stub answers as the code before the planner computed it -- every H <= 256 with
// H % 4 == 0 taken, min(8, 512 / row tiles) chunks asked for, rounded to whole 32-deep k-tiles -- and the as_lin_plain_s6 line
// shows the chunks asked for: that output is equal to the one of the commit before lin_plan.cpp.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "as_launch.h"
#include "gemm_internal.h"
#include "rowops.h"

// 1 lin_try declines, 2 lin_out declines, 4 plain_s6 declines, 8 wgrad_multi declines, 16 tokens_fits false, 32 profile on, 64 no device,
// 128 the caller's stream is capturing, 256 as_gemm_f32 and the GRU backward launchers consume an armed stop event as the real
// ones do, 512 (main() only) the calls go to a stream handle the library has no state for, 1024 the layer-0 recurrence with
// token sums fails to launch (the backward returns its error from inside a fork's scope)
int g_mode = 0;
static void* const EXT_EVENT = (void*)0x5550;   // as_opts.fold_wait_event
static const void* g_seen[2][64];
static int g_nseen[2];
static void put_handle(char kind, const void* h) {
    if (!h) { printf("%c- ", kind); return; }
    if (h == EXT_EVENT) { printf("Eext "); return; }
    const int k = kind == 'E';
    int i = 0;
    while (i < g_nseen[k] && g_seen[k][i] != h) ++i;
    if (i == g_nseen[k]) { if (i == 64) abort(); g_seen[k][g_nseen[k]++] = h; }
    printf("%c%d ", kind, i);
}
void put1(hipStream_t s) { put_handle('S', s); }
void put1(hipEvent_t e) { put_handle('E', e); }
static void put(const void* v, size_t n) { const unsigned char* p = (const unsigned char*)v; for (size_t i = 0; i < n; ++i) printf("%02x", p[i]); printf(" "); }
template <class T> void put1(const T& v) { put(&v, sizeof(T)); }
template <class... T> void logc(const char* name, const T&... a) { printf("%s ", name); (put1(a), ...); printf("\n"); }
static void slab_line(const float* slab, hipStream_t s) { if (slab) logc("@slab", slab, s); }
static void* g_stop = nullptr;
static void carry(hipStream_t s) { if ((g_mode & 256) && g_stop) { logc("@carry", (hipEvent_t)g_stop, s); g_stop = nullptr; } }

int as_dropout(const float* a, float* b, long c, float d, unsigned long long e, hipStream_t s) { logc("as_dropout", a, b, c, d, e, s); return 0; }
int as_lin_try(const as_lin* a, hipStream_t s) { logc("as_lin_try", *a, s); return (g_mode & 1) ? 0 : 1; }
int as_unfold3(const float* const a[3], const float* const b[3], const float* const c[3], const float* const d[3], const float* const e[3],
               float* const f[3], float* const g[3], float* const h[3], const int R[3], const int K[3], int heads, hipStream_t s, int count) {
    printf("as_unfold3 "); for (int i = 0; i < count; ++i) { put1(a[i]); put1(b[i]); put1(c[i]); put1(d[i]); put1(e[i]); put1(f[i]); put1(g[i]); put1(h[i]); put1(R[i]); put1(K[i]); }
    put1(heads); put1(s); put1(count); printf("\n"); return 0; }
int as_emb_grads(const float* a, const float* b, const float* c, int d, int e, int f, float* g, float* h, float* i, hipStream_t s) { logc("as_emb_grads", a, b, c, d, e, f, g, h, i, s); return 0; }
void as_set_error(const char* fmt, ...) { printf("as_set_error %s\n", fmt); }
int as_loss_final(const float* a, int b, float c, float* d, hipStream_t s) { logc("as_loss_final", a, b, c, d, s); return 0; }
int as_emit_planes(const as_planes_job* j, int n, hipStream_t s) { printf("as_emit_planes "); for (int i = 0; i < n; ++i) { put1(j[i].B); put1(j[i].n_stride); put1(j[i].k_stride); put1(j[i].batch_stride); put1(j[i].batch); put1(j[i].N); put1(j[i].K); put1(j[i].rows_pad); put1(j[i].Kpad); put1(j[i].out); } put1(n); put1(s); printf("\n"); return 0; }
int as_gather_rows(const float* a, const int64_t* b, long c, int d, long e, int f, float* g, hipStream_t s, int V) { logc("as_gather_rows", a, b, c, d, e, f, g, s, V); return 0; }
int as_lin_out_try(const as_lin_out* a, int* n, hipStream_t s) { logc("as_lin_out_try", *a, s); if (g_mode & 2) return 0; if (n) *n = a->tgt ? 5 : 0; return 1; }
int as_sigmoid_bwd(const float* a, const float* b, float* c, long d, hipStream_t s) { logc("as_sigmoid_bwd", a, b, c, d, s); return 0; }
int as_token_table(const float* a, const float* b, const float* c, int d, int e, int f, float* g, hipStream_t s) { logc("as_token_table", a, b, c, d, e, f, g, s); return 0; }
int as_wgrad_multi(const as_wgrad_job* j, int n, float* slab, long sf, int cu, hipStream_t s, bool exact) {
    printf("as_wgrad_multi "); for (int i = 0; i < n; ++i) put1(j[i]); put1(n); put1(slab); put1(sf); put1(cu); put1(s); put1(exact); printf("\n"); slab_line(slab, s); return (g_mode & 8) ? 0 : 1; }
as_lin_env as_lin_env_of(hipStream_t, bool) { return as_lin_env{AS_ARITH_BF16X6, true, true, false, AS_LIN_LDS_MI355X}; }
#ifdef DX1_BEFORE_PLANNER
static int dx1_want(const as_lin* a) { const int t = (a->M + 63) / 64, w = 512 / (t > 1 ? t : 1); return w > 8 ? 8 : w < 1 ? 1 : w; }
void as_lin_plain_plan_make(const as_lin* a, int, int, const as_lin_env*, as_lin_plan* p) {
    *p = as_lin_plan{};
    if (a->N > 256 || a->N % 4) return;
    const int kchunk = ((a->K + dx1_want(a) - 1) / dx1_want(a) + 31) / 32 * 32;
    p->family = AS_LIN_PLAIN; p->ksplit = (a->K + kchunk - 1) / kchunk;
}
int as_lin_plain_s6(const as_lin* a, int k, long c, hipStream_t s, int w) { logc("as_lin_plain_s6", *a, k == AS_LIN_KSPLIT_AUTO ? dx1_want(a) : k, c, s, w); return (g_mode & 4) ? 0 : 1; }
#else
int as_lin_plain_s6(const as_lin* a, int k, long c, hipStream_t s, int w) { logc("as_lin_plain_s6", *a, k, c, s, w); return (g_mode & 4) ? 0 : 1; }
#endif
int as_sum_partials(const float* a, long b, int c, float* d, hipStream_t s) { logc("as_sum_partials", a, b, c, d, s); return 0; }
int as_token_segsum(const float* a, const int64_t* b, long c, int d, long e, int f, int g, float* h, hipStream_t s, float* i, long j) { logc("as_token_segsum", a, b, c, d, e, f, g, h, s, i, j); slab_line(i, s); return 0; }
int as_normalize_bwd(const float* a, const float* b, const float* c, const float* d, float* e, long f, int g, hipStream_t s, const unsigned long long* h, int i, long j) { logc("as_normalize_bwd", a, b, c, d, e, f, g, s, h, i, j); return 0; }
int as_normalize_fwd(const float* a, float* b, float* c, long d, int e, hipStream_t s, unsigned long long* f) { logc("as_normalize_fwd", a, b, c, d, e, s, f); return 0; }
bool as_profile_active() { return g_mode & 32; }
int as_count_bad_tokens(const int64_t* a, long b, int c, long d, int e, int* f, hipStream_t s) { logc("as_count_bad_tokens", a, b, c, d, e, f, s); return 0; }
// the slot's owner: only what changes its content is printed (arming an empty slot with nothing, or emptying an empty one, is nothing)
void as_stop_event_set_raw(void* e) { if (e != g_stop) logc("slot=", (hipEvent_t)e); g_stop = e; }
void* as_stop_event_take_raw() { void* e = g_stop; g_stop = nullptr; if (e) logc("slot>", (hipEvent_t)e); return e; }
bool as_gru_bwd_tokens_fits(int a, int b, int c) { return !(g_mode & 16); }
int as_gru_bidir_bwd_tokens(const float* a, const float* b, const float* c, const float* d, const int32_t* e, int f, int g, int h, float* i, const int64_t* j, int64_t k, int l, float* m, hipStream_t s) { logc("as_gru_bidir_bwd_tokens", a, b, c, d, e, f, g, h, i, j, k, l, m, s); if (g_mode & 1024) return AS_ERR_UNSUPPORTED; carry(s); return 1; }
int as_gru_bidir_fwd_tokens(const float* a, const int64_t* b, int64_t c, int d, const float* e, const float* f, const int32_t* g, int h, int i, int j, float* k, float* l, hipStream_t s) { logc("as_gru_bidir_fwd_tokens", a, b, c, d, e, f, g, h, i, j, k, l, s); return 0; }
int as_fold(const float* a, const float* b, const float* c, const float* d, float* e, float* f, int g, int h, int i, hipStream_t s, int j) { logc("as_fold", a, b, c, d, e, f, g, h, i, s, j < h ? h : j /* what reaches the kernel: Rpad < R -> R */); return 0; }
AsProfScope::AsProfScope(const char* name, hipStream_t st) : name_(name), st_(st), a_(nullptr), b_(nullptr) { printf("prof< %s ", name); put1(st); printf("\n"); }
AsProfScope::~AsProfScope() { printf("prof> %s\n", name_); }
extern "C" {
int as_euclid_masked_fwd_bwd_presigmoid(const float* a, const float* b, int64_t c, const int32_t* d, int32_t e, int32_t f, int32_t g, int32_t h, float i, float* j, float* k, float* l, void* s) { logc("as_euclid_presig", a, b, c, d, e, f, g, h, i, j, k, l, (hipStream_t)s); return 0; }
int32_t as_euclid_masked_partials(void) { return 1024; }
int as_gemm_f32(const as_gemm* g, void* s) { logc("as_gemm_f32", *g, (hipStream_t)s); slab_line(g->splitk_ws, (hipStream_t)s); carry((hipStream_t)s); return 0; }
int as_gru_bidir_fwd(const float* a, const int64_t* b, int64_t c, const float* d, const float* e, const int32_t* f, int32_t g, int32_t h, int32_t i, float* j, float* k, void* s) { logc("as_gru_bidir_fwd", a, b, c, d, e, f, g, h, i, j, k, (hipStream_t)s); return 0; }
int as_gru_bidir_bwd(const float* a, const float* b, const float* c, const float* d, const int32_t* e, int32_t f, int32_t g, int32_t h, float* i, float* j, void* s) { logc("as_gru_bidir_bwd", a, b, c, d, e, f, g, h, i, j, (hipStream_t)s); carry((hipStream_t)s); return 0; }
// HIP runtime: fake handles, everything logged
static long g_handle = 0x7000;
hipError_t hipGetDevice(int* d) { *d = 0; return (g_mode & 64) ? hipErrorNoDevice : hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned f) { *e = (hipEvent_t)(g_handle += 16); return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned f) { *s = (hipStream_t)(g_handle += 16); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { logc("hipEventRecord", e, s); return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned f) { logc("hipStreamWaitEvent", s, e, f); return hipSuccess; }
hipError_t hipStreamIsCapturing(hipStream_t s, hipStreamCaptureStatus* c) { *c = (g_mode & 128) ? hipStreamCaptureStatusActive : hipStreamCaptureStatusNone; return hipSuccess; }
const char* hipGetErrorString(hipError_t e) { return "err"; }
}

// one entry-point call: "# call <what> v<option set> <caller's stream>" ... "# <what> v<option set> <result> slot <what the call left armed>"
static void* call(const char* what, int v, void* st) { g_nseen[0] = g_nseen[1] = 0; printf("# call %s v%d ", what, v); put1((hipStream_t)st); printf("\n"); return st; }
static void result(const char* what, int v, int rc) { printf("# %s v%d %d slot ", what, v, rc); put1((hipEvent_t)g_stop); printf("\n"); g_stop = nullptr; }

int main(int argc, char** argv) {
    const bool small = argc > 1 && !strcmp(argv[1], "--small");   // one geometry, every mode and option set
    float* P = (float*)0x100000000, *G = (float*)0x200000000, *ws = (float*)0x300000000, *out = (float*)0x400000000, *dout = (float*)0x500000000;
    float* x = (float*)0x600000000, *dx = (float*)0x700000000, *tgt = (float*)0x800000000, *loss = (float*)0x900000000;
    int64_t* tok = (int64_t*)0xa00000000; int32_t* len = (int32_t*)0xb00000000;
    const int modes[] = {0, 1, 2, 3, 4, 8, 15, 16, 32, 64, 64 | 15, 32 | 15, 128, 128 | 512, 128 | 15, 256, 256 | 16, 256 | 15, 256 | 32, 256 | 128, 256 | 128 | 512, 1024};
    const int Hs[] = {128, 64, 52, 7, 300, 32}, Ns[] = {50, 1, 3, 33, 64, 70}, As[] = {3, 1, 11};
    long calls = 0;
    for (int mode : modes) for (int H : Hs) for (int N : Ns) for (int A : As) for (int rows : {37, 512, 6400}) {
        if (small && (H != 128 || N != 50 || A == 1 || rows == 6400)) continue;
        g_mode = mode;
        for (int simple = 0; simple < 2; ++simple) {
            as_dims d{45, A, 64, H, N, simple};
            as_layout L;
            if (as_artspeech_layout(&d, &L) != 0) continue;
            printf("## mode %d H %d N %d A %d rows %d simple %d\n", mode, H, N, A, rows, simple);
            if (simple) {
                result("head_fwd", 0, as_head_fwd(&d, &L, P, x, rows, out, ws, 1, call("head_fwd", 0, (void*)0x40)));
                result("head_bwd", 0, as_head_bwd(&d, &L, P, out, dout, rows, dx, G, ws, call("head_bwd", 0, (void*)0x40)));
            }
            const int B = rows >= 512 ? 4 : 1, T = rows / B;
            for (int v = 0; v < 5; ++v) {   // bit 0 dropout, bit 1 fused criterion (+ deferred layer-2 gradient), 3: overlap off, 4: deferred update
                as_opts o{};
                o.gru_dropout = (v & 1) ? 0.25f : 0.f; o.dropout_seed = 7;
                if (v & 2) { o.loss_targets = tgt; o.loss_tgt_T = T; o.loss_scale = 0.5f; o.loss_out = loss; o.loss_dout = dout; }
                as_opts ob = o; ob.dout_presigmoid = (v & 2) ? 1 : 0; ob.defer_dw2 = (!simple && v == 2) ? 1 : 0;
                if (v == 4) o.fold_wait_event = EXT_EVENT;
                void* st = (mode & 512) ? (void*)0xa0L : (void*)(0x80L + 0x10 * (mode == 3));
                as_set_overlap(v != 3);
                result("fwd", v, as_artspeech_fwd(&d, P, tok, T, len, B, T, out, ws, 1, v ? &o : nullptr, call("fwd", v, st)));
                result("bwd", v, as_artspeech_bwd(&d, P, tok, T, len, B, T, out, dout, G, ws, v ? &ob : nullptr, call("bwd", v, st)));
                if (ob.defer_dw2) result("dw2", v, as_artspeech_dw2(&d, P, B, T, G, ws, call("dw2", v, st)));
                calls += 2;
            }
        }
    }
    fprintf(stderr, "entry-point call pairs: %ld\n", calls);
    return 0;
}
