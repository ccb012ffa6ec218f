// C ABI (include/aqc_hip.h): single-lane MPS states into dense vectors and into blocks of amplitudes, many states per call.
// Rules: aqc_mps_tovec_rule.h; kernels of the fused route: aqc_mps_tovec.hip; the gemm route is the chain of products of the workspace's
// mps_to_vec (aqc_ws_extra.cpp) on the states' own site pointers, without a workspace.  The skeleton of the call: aqc_mps_call.h.
#include <algorithm>
#include <atomic>
#include <memory>
#include <vector>

#include "aqc_mps_call.h"
#include "aqc_mps_tovec_rule.h"

using namespace aqc;

namespace {

static_assert(kMpsToVecByRule == kMpsByRule && kMpsToVecFused == kMpsFused, "resolve_route");
enum { kSites, kBufs, kDims };                        // the sections of a state's record in the call's table
enum { kLow0, kLow1, kHigh0, kHigh1, kOut, kNumBufs };

std::atomic<size_t> g_budget{kMpsToVecBudget};        // aqc_mps_to_vec_budget: tests lower it to run many chunks on few lanes
thread_local double g_outer_ms = -1.0;                // aqc_mps_to_vec_outer_ms

struct Call {
    int n = 0, k = 0, nstates = 0, device = 0, method = 0;
    bool blocks = false;
    long long high_rows = 0;                          // 2^(n-k), or the listed rows
    const unsigned char* high_bits = nullptr;         // blocks: host, [rows][n - k]
};

// what one group of gemm lanes keeps alive until the chunk's synchronisation
struct GemmWork {
    DevBuf<double2> scratch;
    DevBuf<const void*> tabs;
};

// The chain of mps_to_vec_batch_uniform for states of equal bonds: left half L [2^h][chi] (a new site is the next higher bit), right half
// Rt [2^(n-h)][chi] (a new site is the lowest bit), out = Rt L^T; every step one launch for all states of the group
int run_gemm_group(const std::vector<const MpsView*>& g, const std::vector<double2*>& outs, int n, GemmWork& w, hipStream_t st, int* launches) {
    const int count = (int)g.size(), h = n / 2, mh = n - h;
    const std::vector<int>& dims = g[0]->dims;
    if (h == 0) {   // n = 1: the state is the site tensor itself, [b][1][1]
        for (int i = 0; i < count; ++i) HIP_OK(hipMemcpyAsync(outs[i], g[i]->t[0], sizeof(double2) * 2, hipMemcpyDeviceToDevice, st));
        return 0;
    }
    size_t need_l = 2, need_r = 2;
    for (int q = 0; q < h; ++q) need_l = std::max(need_l, ((size_t)2 << q) * dims[q + 1]);
    for (int q = n - 1; q >= h; --q) need_r = std::max(need_r, ((size_t)2 << (n - 1 - q)) * dims[q]);
    const size_t per = 2 * need_l + 2 * need_r;
    if (w.scratch.alloc(per * (size_t)count)) return 1;
    std::vector<const void*> tabs;
    auto table = [&](auto fn) { const size_t at = tabs.size(); for (int i = 0; i < count; ++i) tabs.push_back(fn(i)); return at; };
    auto lb = [&](int i, int k) { return (const void*)(w.scratch + per * (size_t)i + need_l * (size_t)k); };
    auto rb = [&](int i, int k) { return (const void*)(w.scratch + per * (size_t)i + 2 * need_l + need_r * (size_t)k); };
    auto site = [&](int i, int q) { return (const void*)g[i]->t[q]; };
    struct Step { int kind, q; size_t a, b, c; };   // offsets (in pointers) of the three tables inside the upload
    std::vector<Step> steps;
    for (int q = 1; q < h; ++q) {       // left part: L_q = L_{q-1} T_q, both values of the site's bit (inner = 2)
        Step s{0, q, 0, 0, 0};
        s.a = q == 1 ? table([&](int i) { return site(i, 0); }) : table([&](int i) { return lb(i, (q - 1) & 1); });
        s.b = table([&](int i) { return site(i, q); });
        s.c = table([&](int i) { return lb(i, q & 1); });
        steps.push_back(s);
    }
    for (int q = n - 2; q >= h; --q) {  // right part: Rt_0 = the last site as it is stored; Rt_j[2 c + b] = Rt_{j-1}[c] T_q[b]^T
        const int j = n - 1 - q;
        Step s{2, q, 0, 0, 0};
        s.a = j == 1 ? table([&](int i) { return site(i, n - 1); }) : table([&](int i) { return rb(i, (j - 1) & 1); });
        s.b = table([&](int i) { return site(i, q); });
        s.c = table([&](int i) { return rb(i, j & 1); });
        steps.push_back(s);
    }
    Step fin{3, 0, 0, 0, 0};
    fin.a = mh == 1 ? table([&](int i) { return site(i, n - 1); }) : table([&](int i) { return rb(i, (mh - 1) & 1); });
    fin.b = h == 1 ? table([&](int i) { return site(i, 0); }) : table([&](int i) { return lb(i, (h - 1) & 1); });
    fin.c = table([&](int i) { return (const void*)outs[i]; });
    steps.push_back(fin);
    if (w.tabs.upload(tabs)) return 1;
    const void* const* T = w.tabs;
    for (const Step& s : steps) {
        if (s.kind == 0) {
            const int q = s.q, rows = 1 << q, kk = dims[q], nn = dims[q + 1];
            HIP_OK(launch_zgemm_tables(rows, nn, kk, T + s.a, kk, T + s.b, nn, (void* const*)(T + s.c), nn, 0, (size_t)kk * nn, (size_t)rows * nn, count, 2, st));
        } else if (s.kind == 2) {   // C rows 2 c + b: ldc = 2 chil, the bit's block starts chil further; B = T_q[b] stored [chil][chir], used transposed
            const int q = s.q, j = n - 1 - q, cols = 1 << j, chil = dims[q], chir = dims[q + 1];
            HIP_OK(launch_zgemm_tables(cols, chil, chir, T + s.a, chir, T + s.b, chir, (void* const*)(T + s.c), 2 * chil, 0, (size_t)chil * chir, (size_t)chil,
                                       count, 2, st, 1));
        } else {                    // out [2^mh][2^h] = Rt [2^mh][chi] . L^T, L stored [2^h][chi]
            const int chi = dims[h];
            HIP_OK(launch_zgemm_tables(1 << mh, 1 << h, chi, T + s.a, chi, T + s.b, chi, (void* const*)(T + s.c), 1 << h, 0, 0, 0, count, 1, st, 1));
        }
        ++*launches;
    }
    return 0;
}

struct Stores {
    hipEvent_t ev0 = nullptr, ev1 = nullptr;          // around the outer product of a chunk
    ~Stores() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
    DevBuf<double2> out;                              // the output lanes of a chunk back to back, then its halves: one allocation
    DevBuf<unsigned char> bits;
    MpsTable table;
    std::vector<std::unique_ptr<GemmWork>> gemm;      // of the chunk in flight
};

// the chunks of the call: launches, downloads and one synchronisation each
int run_chunks(const Call& c, const std::vector<MpsView>& views, const std::vector<int>& lane_state, const std::vector<int>& routes, int chunk,
               Stores& s, hipStream_t st, double* out, int* launches) {
    const size_t lanes = views.size(), out_elems = (size_t)c.high_rows << c.k;
    const bool distinct = lanes == (size_t)c.nstates;   // then lane i is state i: a chunk's lanes are delivered by one copy
    MpsToVecArgs a{};
    if (s.table.dev) {   // (no table: every state takes the gemm route)
        a.table = s.table.dev;
        a.per = (int)s.table.layout.per;
        a.at_sites = (int)s.table.layout.at[kSites];
        a.at_bufs = (int)s.table.layout.at[kBufs];
        a.at_dims = (int)s.table.layout.at[kDims];
    }
    a.n = c.n;
    a.k = c.k;
    a.low_len = c.k;
    a.high_len = c.blocks ? 0 : c.n - c.k;
    a.low_store = mps_tovec_half_store(a.low_len);
    a.high_store = mps_tovec_half_store(a.high_len);
    a.high_rows = c.high_rows;
    a.high_bits = s.bits;
    const int longer = std::max(a.low_len, a.high_len);
    for (size_t first = 0; first < lanes; first += (size_t)chunk) {   // the chunks share the stores: one stream orders them
        const int count = (int)std::min((size_t)chunk, lanes - first);
        bool any_fused = false;
        for (int i = 0; i < count; ++i) any_fused = any_fused || routes[first + i] == kMpsToVecFused;
        if (any_fused) {
            a.first = (int)first;
            HIP_OK(launch_mps_tovec_head(a, count, st));
            ++*launches;
            for (int j = kMpsToVecHeadSteps; j < longer; ++j) {
                a.step = j;
                HIP_OK(launch_mps_tovec_step(a, count, st));
                ++*launches;
            }
            if (c.blocks) {
                HIP_OK(launch_mps_tovec_rows(a, count, st));
                ++*launches;
            }
            if (!s.ev0) {
                HIP_OK(hipEventCreate(&s.ev0));
                HIP_OK(hipEventCreate(&s.ev1));
            }
            HIP_OK(hipEventRecord(s.ev0, st));
            HIP_OK(launch_mps_tovec_outer(a, count, st));
            HIP_OK(hipEventRecord(s.ev1, st));
            ++*launches;
        }
        std::vector<bool> done(count, false);
        for (int i = 0; i < count; ++i) {   // the gemm lanes of the chunk, grouped by their bonds
            if (done[i] || routes[first + i] != kMpsToVecGemm) continue;
            std::vector<const MpsView*> g;
            std::vector<double2*> outs;
            for (int j = i; j < count; ++j)
                if (!done[j] && routes[first + j] == kMpsToVecGemm && views[first + j].dims == views[first + i].dims) {
                    done[j] = true;
                    g.push_back(&views[first + j]);
                    outs.push_back(s.out + (size_t)j * out_elems);
                }
            s.gemm.emplace_back(new GemmWork());
            if (run_gemm_group(g, outs, c.n, *s.gemm.back(), st, launches)) return 1;
        }
        if (distinct) {
            HIP_OK(hipMemcpyAsync(out + 2 * first * out_elems, s.out, sizeof(double2) * (size_t)count * out_elems, hipMemcpyDeviceToHost, st));
        } else {
            for (int t = 0; t < c.nstates; ++t) {
                const size_t v = (size_t)lane_state[t];
                if (v < first || v >= first + (size_t)count) continue;
                HIP_OK(hipMemcpyAsync(out + 2 * (size_t)t * out_elems, s.out + (v - first) * out_elems, sizeof(double2) * out_elems, hipMemcpyDeviceToHost, st));
            }
        }
        HIP_OK(hipStreamSynchronize(st));   // the one synchronisation of the chunk: its stores are the next chunk's
        float ms = 0.0f;
        if (any_fused && hipEventElapsedTime(&ms, s.ev0, s.ev1) == hipSuccess) g_outer_ms = (g_outer_ms < 0.0 ? 0.0 : g_outer_ms) + ms;
        s.gemm.clear();
    }
    return 0;
}

int run(aqc_mps* const* states, const Call& c, double* out, int32_t* info) {
    const int n = c.n, nstates = c.nstates;
    HIP_OK(hipSetDevice(c.device));
    hipStream_t st = mps_stream(states[0]);
    std::vector<MpsView> views;
    std::vector<int> lane_state;
    if (view_states(states, (size_t)nstates, n, views, lane_state)) return 1;
    std::vector<int> routes(views.size(), 0);
    bool any_fused = false;
    for (int s = 0; s < nstates; ++s) {
        const MpsView& v = views[lane_state[s]];
        int& route = routes[lane_state[s]];
        if (route) continue;
        if (c.blocks && v.max_bond > kMpsObsFusedCap)
            return failf("blocks of amplitudes take the fused route only: bond dimensions up to %d; state %d has %d", (int)kMpsObsFusedCap, s, v.max_bond);
        if ((route = resolve_route(c.method, mps_tovec_route(n, v.dims.data()), v.max_bond, kMpsObsFusedCap, "state", s)) < 0) return 1;
        any_fused = any_fused || route == kMpsToVecFused;
    }
    const size_t lanes = views.size(), out_elems = (size_t)c.high_rows << c.k;
    const size_t lane_bytes = mps_tovec_lane_bytes(c.k, (size_t)c.high_rows), budget = g_budget.load();
    const int chunk = mps_tovec_chunk(lane_bytes, lanes, budget);
    if (chunk < 1)
        return failf("one state of %d qubits needs %zu bytes of device memory for its amplitudes and halves, the budget is %zu (aqc_mps_to_vec_budget)", n,
                     lane_bytes, budget);
    Stores s;
    g_outer_ms = -1.0;
    int fused_bond = 1;                               // the stores of the halves are sized by the largest bond of the fused states
    for (size_t v = 0; v < lanes; ++v)
        if (routes[v] == kMpsToVecFused) fused_bond = std::max(fused_bond, views[v].max_bond);
    const size_t low_elems = mps_tovec_half_elems(mps_tovec_low_rows(c.k), fused_bond), high_elems = mps_tovec_half_elems((size_t)c.high_rows, fused_bond);
    const size_t high_stores = c.blocks ? 1 : 2, half_elems = any_fused ? 2 * low_elems + high_stores * high_elems : 0;
    if (s.out.alloc((size_t)chunk * (out_elems + half_elems))) return 1;
    if (any_fused) {
        if (c.blocks && s.bits.upload(std::vector<unsigned char>(c.high_bits, c.high_bits + (size_t)c.high_rows * (n - c.k)))) return 1;
        s.table = MpsTable({mps_table_words((size_t)n), mps_table_words((size_t)kNumBufs), mps_table_ints((size_t)n + 2)}, lanes);
        for (size_t v = 0; v < lanes; ++v) {
            const size_t slot = v % (size_t)chunk;
            std::vector<double2*> bufs(kNumBufs, nullptr);
            bufs[kLow0] = s.out + (size_t)chunk * out_elems + slot * half_elems;
            bufs[kLow1] = bufs[kLow0] + low_elems;
            bufs[kHigh0] = bufs[kLow1] + low_elems;
            bufs[kHigh1] = c.blocks ? nullptr : bufs[kHigh0] + high_elems;
            bufs[kOut] = s.out + slot * out_elems;
            std::vector<int> dims(views[v].dims);
            dims.push_back(routes[v]);
            s.table.put(v, kSites, views[v].t, n);
            s.table.put(v, kBufs, bufs, kNumBufs);
            s.table.put(v, kDims, dims, n + 2);
        }
        if (s.table.upload()) return 1;
    }
    int launches = 0;
    if (finish_call(st, run_chunks(c, views, lane_state, routes, chunk, s, st, out, &launches), c.blocks ? "amplitude blocks" : "conversion")) return 1;
    if (info) {
        for (int t = 0; t < nstates; ++t) info[t] = routes[lane_state[t]];
        info[nstates] = c.k;
        info[nstates + 1] = (int32_t)mps_tovec_chunks(lanes, chunk);
        info[nstates + 2] = launches;
    }
    return 0;
}

}  // namespace

extern "C" {

int aqc_mps_to_vec_route(int n, const int32_t* dims) {
    if (!dims || n < 1) return -1;
    return mps_tovec_route(n, dims);
}

int64_t aqc_mps_to_vec_budget(int64_t bytes) {
    return swap_budget(g_budget, bytes, kMpsToVecBudget);
}

double aqc_mps_to_vec_outer_ms(void) { return g_outer_ms; }

int aqc_mps_to_vec(aqc_mps* const* states, int nstates, int method, double* out, int32_t* info) {
    if (!states || !out) return failf("null argument");
    if (nstates < 1) return failf("at least one state is needed");
    if (!mps_tovec_method_ok(method)) return failf("unknown method %d", method);
    Call c;
    if (check_states(states, nullptr, nstates, 1, &c.n, &c.device)) return 1;
    if (c.n > kMpsToVecMaxQubits) return failf("a dense vector takes at most %d qubits, the states have %d (blocks: aqc_mps_amp_blocks)", (int)kMpsToVecMaxQubits, c.n);
    c.nstates = nstates;
    c.method = method;
    c.k = mps_tovec_split(c.n);
    c.high_rows = (long long)mps_tovec_high_rows(c.n, c.k);
    return run(states, c, out, info);
}

int aqc_mps_amp_blocks(aqc_mps* const* states, int nstates, int low_qubits, int64_t rows, const uint8_t* high_bits, int method, double* out) {
    if (!states || !high_bits || !out) return failf("null argument");
    if (nstates < 1) return failf("at least one state is needed");
    if (!mps_tovec_method_ok(method)) return failf("unknown method %d", method);
    if (method == kMpsToVecGemm) return failf("blocks of amplitudes take the fused route only");
    Call c;
    if (check_states(states, nullptr, nstates, 1, &c.n, &c.device)) return 1;
    if (const char* msg = mps_tovec_check_blocks(c.n, low_qubits, rows)) return failf("%s (%d qubits, low_qubits %d, %lld rows)", msg, c.n, low_qubits, (long long)rows);
    const int width = c.n - low_qubits;
    const long long bad = mps_tovec_bad_bit(high_bits, (size_t)rows * width);
    if (bad >= 0) return failf("row %lld, qubit %lld: a bit is 0 or 1, not %d", bad / width, low_qubits + bad % width, (int)high_bits[bad]);
    c.nstates = nstates;
    c.method = method;
    c.blocks = true;
    c.k = low_qubits;
    c.high_rows = rows;
    c.high_bits = high_bits;
    return run(states, c, out, nullptr);
}

}  // extern "C"
