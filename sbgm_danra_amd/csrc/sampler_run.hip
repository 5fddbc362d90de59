// The step samplers (EM, PC, EDM Heun, DPM-Solver++(2M)) and the RK45 driver: the step tables, one run's hold on the model, the state
// that outlives a call (SamplerStore) and the sbgm_sampler_run* entry points (engine.h says who owns what).
#include <cmath>
#include <cstdio>

#include "engine.h"

struct sbgm_model::EdmArgs { float sigma_min, sigma_max, rho, s_churn, s_tmin, s_tmax, s_noise; };
struct sbgm_model::HeldArgs { const float *known, *mask; };        // constrained sampling: both device [B][1][H][W], used in place
struct sbgm_model::JointArgs { int domain_h, ramp_len; };          // joint tiled sampling: the B tiles are one domain of domain_h x a.domain_w
struct sbgm_model::DpmArgs { float sigma_min, sigma_max, rho, eta, s_noise; };     // DPM-Solver++(2M): eta > 0 is the SDE variant
struct sbgm_model::OdeArgs { double t0, t1, rtol, atol; int per_sample; long long max_steps; const float* x0; int64_t* stats_i; double* stats_d; };

// ---- the state that outlives a call ------------------------------------------------------------------------------------
SamplerStore::~SamplerStore() {
    drop_step_graph();
    if (d_state) (void)hipFree(d_state);
    if (d_table) (void)hipFree(d_table);
    if (d_levels) (void)hipFree(d_levels);
    for (RunBuf* b : {&d_times, &d_rows, &d_tbrun}) if (b->p) (void)hipFree(b->p);
    if (h_stage) (void)hipHostFree(h_stage);
    if (ev_stage) (void)hipEventDestroy(ev_stage);
    if (graph_stream) (void)hipStreamDestroy(graph_stream);
    if (ev_replayed) (void)hipEventDestroy(ev_replayed);
    if (h_done) (void)hipHostFree(h_done);
    for (hipEvent_t e : ev_poll) if (e) (void)hipEventDestroy(e);
}

void SamplerStore::drop_step_graph() {
    if (step_exec && ev_replayed) (void)hipEventSynchronize(ev_replayed);        // a replay of it may still be executing
    if (step_exec) (void)hipGraphExecDestroy(step_exec);
    if (step_graph) (void)hipGraphDestroy(step_graph);
    step_exec = nullptr;
    step_graph = nullptr;
}

int SamplerStore::ensure_step_graph(const StepGraphKey& key, bool recapture, hipStream_t& st, const std::function<int()>& body) {
    if (step_exec != nullptr && !recapture && std::memcmp(&key, &step_key, sizeof key) == 0) return 0;
    drop_step_graph();
    const hipStream_t caller = st;
    st = graph_stream;
    int rc = 0;
    hipError_t e = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) { sbgm_set_error("hipStreamBeginCapture failed: %s", hipGetErrorString(e)); rc = 2; }
    if (rc == 0) {
        rc = body();
        e = hipStreamEndCapture(st, &step_graph);
        if (rc == 0 && (e != hipSuccess || hipGraphInstantiate(&step_exec, step_graph, nullptr, nullptr, 0) != hipSuccess)) {
            sbgm_set_error("hipGraph capture/instantiate failed: %s", hipGetErrorString(e));
            rc = 2;
        }
        if (rc) drop_step_graph();
        else step_key = key;
    }
    st = caller;
    return rc;
}

// torch.linspace(start, end, n) in fp32, as ATen fills it (symmetric about the midpoint)
static std::vector<float> linspace_f32(float start, float end, int n) {
    std::vector<float> v(n);
    if (n == 1) { v[0] = start; return v; }
    const float step = (end - start) / (float)(n - 1);
    const int half = n / 2;
    for (int i = 0; i < n; ++i) v[i] = i < half ? start + step * (float)i : end - step * (float)(n - 1 - i);
    return v;
}

// Step tables, in the reference's precision.  Each builder writes the N rows of its kind into the staging buffer and returns the row
// size and the time of the run's first evaluation.
struct StepTable { size_t row_bytes; float t_first; };

// Euler-Maruyama: torch.linspace times in fp32 (score_sampling.py:96-97, :102-103, :124-125)
static StepTable em_table(void* stage, int N, float sig, float eps, const sbgm_model::EdmArgs*, const sbgm_model::DpmArgs*) {
    StepScalars* tab = static_cast<StepScalars*>(stage);
    const std::vector<float> ts = linspace_f32(1.0f, eps, N);
    const float dt = ts[0] - ts[1];
    for (int i = 0; i < N; ++i) {
        const float g = powf(sig, ts[i]);
        tab[i] = StepScalars{ts[i], g * g, dt, sqrtf(dt) * g, ts[std::min(i + 1, N - 1)]};
    }
    return {sizeof(StepScalars), tab[0].t};
}

// predictor-corrector: np.linspace times in float64, stored as fp32 (score_sampling.py:169-170, :176, :207, :224-227)
static StepTable pc_table(void* stage, int N, float sig, float eps, const sbgm_model::EdmArgs*, const sbgm_model::DpmArgs*) {
    StepScalars* tab = static_cast<StepScalars*>(stage);
    std::vector<double> ts(N);
    const double step = ((double)eps - 1.0) / (double)(N - 1);
    for (int i = 0; i < N; ++i) ts[i] = 1.0 + (double)i * step;
    ts[N - 1] = (double)eps;
    const float dt = (float)(ts[0] - ts[1]);
    for (int i = 0; i < N; ++i) {
        const float tf = (float)ts[i];
        const float g = powf(sig, tf);
        tab[i] = StepScalars{tf, g * g, dt, sqrtf((g * g) * dt), (float)ts[std::min(i + 1, N - 1)]};
    }
    return {sizeof(StepScalars), tab[0].t};
}

// The Karras ladder of the few-step samplers for the VE SDE std(t) = sqrt((sigma^2t - 1) / (2 ln sigma)): sigma_0 .. sigma_{N-1} between
// sigma_min and sigma_max (<= 0: the trained range [std(eps), std(1)]; other values are clipped to it), sigma_N = 0, and t(sigma) =
// log1p(2 ln sigma * s^2) / (2 ln sigma) clamped to [eps, 1].  float64 throughout.
struct KarrasLadder {
    double ls, lo, hi, eps;
    std::vector<double> sg;                                // [N + 1]
    KarrasLadder(int N, double sig, double eps_, float sigma_min, float sigma_max, float rho_) : ls(std::log(sig)), eps(eps_), sg(N + 1) {
        auto std_of = [&](double t) { return std::sqrt(std::expm1(2.0 * t * ls) / (2.0 * ls)); };
        lo = std_of(eps); hi = std_of(1.0);
        const double smin = sigma_min > 0 ? std::min(hi, std::max(lo, (double)sigma_min)) : lo;
        const double smax = sigma_max > 0 ? std::min(hi, std::max(lo, (double)sigma_max)) : hi;
        const double rho = rho_, a0 = std::pow(smax, 1.0 / rho), a1 = std::pow(smin, 1.0 / rho);
        for (int i = 0; i < N; ++i) sg[i] = std::pow(a0 + (double)i / (double)(N - 1) * (a1 - a0), rho);
        sg[0] = smax; sg[N - 1] = smin; sg[N] = 0.0;       // the ends exactly (the power round trip is off by an ulp)
    }
    double t_of(double s) const {                          // clamped in sigma too: sigma >= std(1) is t = 1 exactly
        return s >= hi ? 1.0 : s <= lo ? eps : std::min(1.0, std::max(eps, std::log1p(2.0 * ls * s * s) / (2.0 * ls)));
    }
};

// EDM Heun step table (Karras et al. 2022, Alg. 2): the ladder with the churn gamma_i.  Stored as fp32: score_sampling.edm_heun_schedule.
static StepTable edm_table(void* stage, int N, float sig, float eps, const sbgm_model::EdmArgs* edm, const sbgm_model::DpmArgs*) {
    const sbgm_model::EdmArgs& e = *edm;
    EdmStep* tab = static_cast<EdmStep*>(stage);
    const KarrasLadder k(N, (double)sig, (double)eps, e.sigma_min, e.sigma_max, e.rho);
    const std::vector<double>& sg = k.sg;
    const double gmax = std::min((double)e.s_churn / (double)N, std::sqrt(2.0) - 1.0);
    for (int i = 0; i < N; ++i) {
        double g = (e.s_tmin <= sg[i] && sg[i] <= e.s_tmax) ? gmax : 0.0;
        g = std::min(g, sg[0] / sg[i] - 1.0);
        const double sh = sg[i] * (1.0 + g);
        tab[i] = EdmStep{(float)sg[i], (float)sh, (float)sg[i + 1], (float)k.t_of(sh), (float)k.t_of(sg[i + 1]),
                         (float)((double)e.s_noise * std::sqrt(std::max(0.0, sh * sh - sg[i] * sg[i])))};
    }
    return {sizeof(EdmStep), tab[0].t_hat};
}

// DPM-Solver++(2M) step table (Lu et al. 2022; eta > 0: 2M SDE, midpoint form) on the same ladder, alpha = 1: the coefficients of
// x_{i+1} = c_x x_i + c_0 D_i + c_1 D_{i-1} + c_z z_i (kernels.h: DpmStep).  Stored as fp32: score_sampling.dpmpp_2m_schedule.
static StepTable dpm_table(void* stage, int N, float sig, float eps, const sbgm_model::EdmArgs*, const sbgm_model::DpmArgs* dpm) {
    const sbgm_model::DpmArgs& d = *dpm;
    DpmStep* tab = static_cast<DpmStep*>(stage);
    const KarrasLadder k(N, (double)sig, (double)eps, d.sigma_min, d.sigma_max, d.rho);
    const std::vector<double>& sg = k.sg;
    const double eta = d.eta;
    double h_prev = 0.0;
    for (int i = 0; i < N; ++i) {
        double c_x = 0.0, c_0 = 1.0, c_1 = 0.0, c_z = 0.0;   // the last step: x_N = D_{N-1}
        if (i + 1 < N) {
            const double h = std::log(sg[i] / sg[i + 1]), a = -std::expm1(-(1.0 + eta) * h);
            c_x = sg[i + 1] / sg[i] * std::exp(-eta * h);
            c_0 = a;
            if (i >= 1) {
                const double r = h_prev / h;
                c_0 = a * (1.0 + 1.0 / (2.0 * r));
                c_1 = -a / (2.0 * r);
            }
            c_z = (double)d.s_noise * sg[i + 1] * std::sqrt(std::max(0.0, -std::expm1(-2.0 * eta * h)));
            h_prev = h;
        }
        tab[i] = DpmStep{(float)sg[i], (float)k.t_of(sg[i]), (float)k.t_of(sg[i + 1]), (float)c_x, (float)c_0, (float)c_1, (float)c_z};
    }
    return {sizeof(DpmStep), tab[0].t};
}

// What differs between the step-sampler kinds outside the step body, once: plain data that sampler() and SamplerStore::stage read.
struct StepKind {
    int kind;                                    // SBGM_SAMPLER_*
    bool edm_args, dpm_args;                     // the scalar block its entry point passes
    StepTable (*table)(void* stage, int N, float sig, float eps, const sbgm_model::EdmArgs*, const sbgm_model::DpmArgs*);   // + its row size
    float (*row_t)(const void* tab, int i);      // the evaluation time of step i in the staged table (null: more than one per step)
    float (*row_sigma)(const void* tab, int i);  // the noise level of step i (null: std(row_t), the table stores none)
    int state_slab, result_slab;                 // where the state starts, and which slab is copied to `out` (slab 0: the network input)
    int tail;                                    // eager last steps that write `out` themselves
    bool keeps_rows;                             // a run without labels keeps its time rows (one evaluation per step, at the table's time)
    bool level_table;                            // a constrained run needs the hold levels as a table beside the step table
    bool hold_draw0;                             // while it draws no noise per step, its held pixels carry the run's draw 0
    bool key_corrector;                          // cfg_scale_corrector and snr * sqrt(n) are baked into the captured step
};
template <class Row> static float row_time(const void* tab, int i) { return static_cast<const Row*>(tab)[i].t; }
template <class Row> static float row_level(const void* tab, int i) { return static_cast<const Row*>(tab)[i].sigma; }
// EM / PC: the result is the x_mean slab; EDM Heun keeps its state x / x_hat in x_mean and its tail, the Euler-only last step, writes
// `out` itself (it evaluates at two times per step and keeps its launches); 2M keeps its state in the network input (its history
// D_{i-1} in x_mean) and evaluates once per step, at its table's time, so it keeps its rows like EM / PC.
static const StepKind STEP_KINDS[] = {
    {SBGM_SAMPLER_EM, false, false, em_table, row_time<StepScalars>, nullptr, 0, 2, 0, true, true, false, true},
    {SBGM_SAMPLER_PC, false, false, pc_table, row_time<StepScalars>, nullptr, 0, 2, 0, true, true, false, true},
    {SBGM_SAMPLER_EDM_HEUN, true, false, edm_table, nullptr, row_level<EdmStep>, 2, -1, 1, false, false, true, false},
    {SBGM_SAMPLER_DPMPP_2M, false, true, dpm_table, row_time<DpmStep>, row_level<DpmStep>, 0, 0, 0, true, true, true, false},
};
static const StepKind* step_kind(int kind, bool edm_args, bool dpm_args) {
    for (const StepKind& k : STEP_KINDS)
        if (k.kind == kind && k.edm_args == edm_args && k.dpm_args == dpm_args) return &k;
    return nullptr;
}

// What a call asks SamplerStore::stage for, and the device pointers its step gets back
struct StepStage {
    const sbgm_sampler_args& a;
    const sbgm_model::EdmArgs* edm;
    const sbgm_model::DpmArgs* dpm;
    bool held, keep_rows;
    int BE;
    StepTable tab{};
    float sigma0 = 0.f;                          // the first row's noise level, where the kind's table stores one
    const void* table = nullptr;
    const HoldLevels* levels = nullptr;
    TimeRows rows{};
};

// The step table and the initial state, written into the pinned staging buffer and uploaded from there; the hold levels; the time rows
int SamplerStore::stage(const sbgm_model& m, const StepKind& kind, StepStage& s, hipStream_t st) {
    const sbgm_sampler_args& a = s.a;
    const int N = a.num_steps;
    static_assert(sizeof(DpmStep) >= sizeof(EdmStep) && sizeof(EdmStep) >= sizeof(StepScalars), "the staging buffer is sized for the largest row");
    const size_t stage_need = (sizeof(DpmStep) + sizeof(HoldLevels) + sizeof(float)) * (size_t)N + sizeof(SamplerState);
    if (stage_pending) {                                   // the previous call's upload still reads the buffer (normally long done)
        SBGM_HIP(hipEventSynchronize(ev_stage));
        stage_pending = false;
    }
    if (h_stage_bytes < stage_need) {
        if (h_stage) SBGM_HIP(hipHostFree(h_stage));
        h_stage = nullptr;
        h_stage_bytes = std::max(stage_need, (sizeof(DpmStep) + sizeof(HoldLevels) + sizeof(float)) * (size_t)4096 + sizeof(SamplerState));
        SBGM_HIP(hipHostMalloc(reinterpret_cast<void**>(&h_stage), h_stage_bytes, hipHostMallocDefault));
    }
    if (!ev_stage) SBGM_HIP(hipEventCreateWithFlags(&ev_stage, hipEventDisableTiming));
    const float sig = m.cfg.sigma;
    s.tab = kind.table(h_stage, N, sig, a.eps, s.edm, s.dpm);
    if (kind.row_sigma) s.sigma0 = kind.row_sigma(h_stage, 0);
    const size_t tab_bytes = s.tab.row_bytes * (size_t)N;
    if (table_bytes < tab_bytes) {                         // roomy: a new table address invalidates the cached step graph
        if (d_table) SBGM_HIP(hipFree(d_table));
        d_table = nullptr;
        const size_t cap = std::max(tab_bytes, sizeof(StepScalars) * 4096);
        SBGM_HIP(hipMalloc(&d_table, cap));
        table_bytes = cap;
    }
    SamplerState* state0 = reinterpret_cast<SamplerState*>(h_stage + tab_bytes);
    *state0 = SamplerState{0ull, 0ull, (unsigned long long)a.seed, (unsigned long long)N};
    SBGM_HIP(hipMemcpyAsync(d_table, h_stage, tab_bytes, hipMemcpyHostToDevice, st));
    SBGM_HIP(hipMemcpyAsync(d_state, state0, sizeof(SamplerState), hipMemcpyHostToDevice, st));
    s.table = d_table;
    // Constrained EM / PC run: the levels its held pixels are re-noised to, std(t_i) and std(t_{i+1}) (0 after the last step) with std =
    // marginal_prob_std in double at the table's fp32 times, as a table parallel to the step table (EDM Heun: EdmStep has sigma_next).
    // 2M: the ladder itself, sigma_i and sigma_{i+1} as the table stores them.
    if (s.held && kind.level_table) {
        if (levels_rows < (size_t)N) {
            if (d_levels) SBGM_HIP(hipFree(d_levels));
            d_levels = nullptr;
            levels_rows = std::max<size_t>(N, 4096);
            SBGM_HIP(hipMalloc(reinterpret_cast<void**>(&d_levels), levels_rows * sizeof(HoldLevels)));
        }
        HoldLevels* lv = reinterpret_cast<HoldLevels*>(h_stage + tab_bytes + sizeof(SamplerState));
        const double lsd = std::log((double)sig);
        for (int i = 0; i < N; ++i)
            lv[i].cur = kind.row_sigma ? kind.row_sigma(h_stage, i)
                                       : (float)std::max(std::sqrt(std::expm1(2.0 * (double)kind.row_t(h_stage, i) * lsd) / (2.0 * lsd)), 1e-5);
        for (int i = 0; i < N; ++i) lv[i].next = i + 1 < N ? lv[i + 1].cur : 0.f;
        SBGM_HIP(hipMemcpyAsync(d_levels, lv, sizeof(HoldLevels) * (size_t)N, hipMemcpyHostToDevice, st));
        s.levels = d_levels;
    }
    // Time rows: an EM / PC run without labels evaluates every sample at the table's time of the step, so the nine
    // time-bias vectors of all N steps are computed here, once per call and outside the captured step, by the forward's own two kernels
    // with the N table times as their "samples" (a row does not depend on the other rows: bit-equal to what the step would compute);
    // the step's advance then copies row step + 1 into tbrun.  EDM Heun evaluates at two times per step and keeps its launches; a 2M
    // step evaluates once, at its table's time, and keeps its rows like EM / PC.
    if (s.keep_rows) {
        int off4[10];
        const int TB = m.time_row_layout(off4);
        SBGM_CHECK(TB > 0, "sampler: time-bias widths must be multiples of 4");
        constexpr int CHUNK = 512;                         // rows per launch: bounds the embedding scratch, taken from the idle workspace
        const size_t scratch = (size_t)5 * std::min(N, CHUNK) * m.D * 4;
        SBGM_CHECK(scratch <= m.ws_bytes, "sampler: workspace too small for the time-row scratch");
        if (d_times.need((size_t)N * 4, (size_t)4096 * 4) || d_rows.need((size_t)N * TB * 4, (size_t)1024 * TB * 4) ||
            d_tbrun.need((size_t)s.BE * TB * 4, (size_t)64 * TB * 4)) return 1;
        float* h_times = reinterpret_cast<float*>(h_stage + tab_bytes + sizeof(SamplerState) + sizeof(HoldLevels) * (size_t)N);
        for (int i = 0; i < N; ++i) h_times[i] = kind.row_t(h_stage, i);
        SBGM_HIP(hipMemcpyAsync(d_times.p, h_times, (size_t)N * 4, hipMemcpyHostToDevice, st));
        for (int r0 = 0; r0 < N; r0 += CHUNK) {
            float* out[9];
            for (int i = 0; i < 9; ++i) out[i] = d_rows.f() + (size_t)r0 * TB + off4[i] * 4;
            if (m.time_biases(d_times.f() + r0, nullptr, std::min(CHUNK, N - r0), reinterpret_cast<float*>(m.ws), out, TB, st)) return 1;
        }
        TimeRows& trows = s.rows;
        trows.rows = d_rows.f(); trows.tbrun = d_tbrun.f(); trows.n = 9; trows.BE = s.BE;
        for (int i = 0; i <= 9; ++i) trows.off4[i] = off4[i];
        if (sbgm_launch_time_rows_bcast(trows, 0, st)) return 1;
    }
    SBGM_HIP(hipEventRecord(ev_stage, st));               // no host wait: the copies read pinned memory this handle owns
    stage_pending = true;
    return 0;
}

// Condition tensors of a run's network evaluations: the caller's, or with guidance (guided_score_fn :27-43) per-call copies of 2B rows
// whose second half is the unconditional input (null class 0, zero cond_img, geo fields with their mask channel zeroed).  The copies
// are freed on every exit path, after the stream has drained.
struct SamplerConds {
    const int64_t* y;
    const float *cond, *lsm, *topo;
    hipStream_t st;
    std::vector<void*> bufs;
    SamplerConds(const sbgm_sampler_args& a, hipStream_t s) : y(a.y), cond(a.cond_img), lsm(a.lsm_cond), topo(a.topo_cond), st(s) {}
    SamplerConds(const SamplerConds&) = delete;
    ~SamplerConds() {
        if (bufs.empty()) return;
        (void)hipStreamSynchronize(st);
        for (void* p : bufs) (void)hipFree(p);
    }
    int add_unconditional(const sbgm_sampler_args& a, const sbgm_model_config& c) {
        const size_t per = (size_t)a.H * a.W, n = (size_t)a.B * per;
        // p -> [p; unconditional half]: zeros, or for a geo field with geo_ch channels a copy, with channel 1 (the mask) zeroed if 2
        auto dup = [&](auto& p, size_t bytes_half, int geo_ch) -> bool {
            void* d = nullptr;
            if (p == nullptr) return true;
            if (hipMalloc(&d, 2 * bytes_half) != hipSuccess) return false;
            bufs.push_back(d);
            (void)hipMemcpyAsync(d, p, bytes_half, hipMemcpyDeviceToDevice, st);
            char* lo = static_cast<char*>(d) + bytes_half;
            if (geo_ch == 0) (void)hipMemsetAsync(lo, 0, bytes_half, st);
            else (void)hipMemcpyAsync(lo, p, bytes_half, hipMemcpyDeviceToDevice, st);
            if (geo_ch == 2) (void)hipMemset2DAsync(lo + per * 4, 2 * per * 4, 0, per * 4, a.B, st);   // NCHW [B][2][H][W]
            p = static_cast<std::remove_reference_t<decltype(p)>>(d);
            return true;
        };
        SBGM_CHECK(dup(y, (size_t)a.B * 8, 0) && dup(cond, n * 4 * c.n_cond_channels, 0) &&
                   dup(lsm, n * 4 * c.n_lsm_channels, c.n_lsm_channels) && dup(topo, n * 4 * c.n_topo_channels, c.n_topo_channels) &&
                   hipGetLastError() == hipSuccess, "sampler: could not allocate the unconditional condition tensors");
        return 0;
    }
};

// What the drivers below share, done once: one sampler call's hold on the model.  open() validates the call and settles the workspace;
// begin() carves the run's persistent buffers off its top (the forward uses the rest), refreshes the derived weights ahead of any
// capture, builds the conditions, the routes and the tiled noise map and takes the buffers out of the forward's reach.  The destructor
// gives the workspace back and ends the routes on every exit path.  Layout from `top` (BE = B, or 2B with guidance): `lead` slabs of
// BE*per floats (slab 0: the network input, rows B.. mirror rows 0..B-1), the time vector [BE], double partials [BE], the kind's
// further slabs, the composed stem's condition term, conv1's condition share for the skip the final mix forms (skip_Sc).
struct SamplerRun {
    sbgm_model* m;
    const sbgm_sampler_args& a;
    hipStream_t st;                  // the caller's stream (ensure_step_graph points it at the capture stream meanwhile)
    const char* who;                 // the driver's name in error texts
    const bool graphed;
    const int B = a.B, H = a.H, W = a.W, slabs = sbgm_model::sampler_slabs(a.kind), lead = a.kind == SBGM_SAMPLER_RK45 ? slabs : 3;
    const bool guided = a.cfg_enabled != 0;
    const int BE = guided ? 2 * B : B;                     // samples per network evaluation
    const size_t per = (size_t)H * W, n = (size_t)B * per, slab = align_up((size_t)BE * per * 4, 256);
    char* top = nullptr;
    size_t saved_ws = 0;             // the model's ws_bytes while the run holds its slabs (0: not held)
    SamplerConds conds{a, st};       // guidance: the unconditional half is built once per run
    NoiseMap nm{};
    const sbgm_model::NoiseRows* plan = nullptr;   // set by the driver before begin(): the run's noise plan (checked by check_plan)
    float* tbrun = nullptr;          // set by an EM / PC driver before begin(): the run keeps its time biases
    ~SamplerRun() { if (saved_ws) m->ws_bytes = saved_ws; m->set_routes(CALL_PLAIN); }
    size_t sc_bytes() const { return a.kind != SBGM_SAMPLER_RK45 ? m->skip_sc_bytes(BE, H, W) : 0; }
    size_t keep() const { return m->sampler_keep(BE, H, W, slabs) + sc_bytes(); }
    float* slab_at(int i) const { return reinterpret_cast<float*>(top + (i < lead ? i * slab : m->slabs_keep(BE, H, W, lead) + (i - lead) * slab)); }
    float* t_vec() const { return reinterpret_cast<float*>(top + lead * slab); }
    double* partials() const { return reinterpret_cast<double*>(top + lead * slab + align_up((size_t)BE * 4, 256)); }
    float* stem_T() const { return reinterpret_cast<float*>(top + m->slabs_keep(BE, H, W, slabs)); }
    float* skip_Sc() const { return reinterpret_cast<float*>(top + m->sampler_keep(BE, H, W, slabs)); }
    int open() {
        SBGM_CHECK(B >= 1 && H >= 32 && W >= 32, "%s: needs B >= 1 and H, W >= 32, got B=%d H=%d W=%d", who, B, H, W);
        SBGM_CHECK(!(guided && a.bn_train), "%s: guidance with train-mode BatchNorm would couple the two halves of the batch", who);
        return m->prepare_ws(BE, H, W, a.bn_train, st, slabs, sc_bytes());
    }
    int begin(bool draws_noise = true) {
        // Graph CAPTURE is illegal on the legacy default stream, so the step is captured on a private stream (capture records, it runs
        // nothing); the replays, the uploads and the final copy go to the caller's stream: ordinary stream-ordered work of the caller.
        if (graphed && !m->store.graph_stream) {
            SBGM_HIP(hipStreamCreateWithFlags(&m->store.graph_stream, hipStreamNonBlocking));
            SBGM_HIP(hipEventCreateWithFlags(&m->store.ev_replayed, hipEventDisableTiming));
        }
        top = m->ws + m->ws_bytes - keep();
        if (m->refresh_derived(st, a.kind != SBGM_SAMPLER_RK45, H, W, a.kind != SBGM_SAMPLER_RK45, BE)) return 1;
        if (guided && conds.add_unconditional(a, m->cfg)) return 1;
        if (a.kind != SBGM_SAMPLER_RK45) {
            // The run's condition term T: the composed filter over the channels that do not change from step to step (lsm, topo, cond_img,
            // in conv1's order after x).  On every call, outside the captured step: a cached step graph is replayed on new condition
            // contents at the same addresses.
            if (m->stem.prepare(*m->conv1.w, *m->conv2.w, m->cin_total, st)) return 1;
            const float *srcs[3] = {conds.lsm, conds.topo, conds.cond}, *term = nullptr;
            const int chs[3] = {m->cfg.n_lsm_channels, m->cfg.n_topo_channels, m->cfg.n_cond_channels};
            for (int i = 0, c0 = 1; i < 3 && m->stem.on; c0 += chs[i++]) {
                if (!chs[i]) continue;
                if (sbgm_launch_conv_stem22(srcs[i], chs[i], c0, m->cin_total, m->stem.wc, nullptr, nullptr, term, nullptr, nullptr, 0, stem_T(), BE, H, W, st)) return 1;
                term = stem_T();
            }
            // The same for the decoder's last skip where the final mix forms it (skip_mix_route): conv1 is linear, so its share over those
            // channels, Sc, is one pack_input with the x slot left zero and one conv1 launch without time bias into the run's buffer,
            // staged through the forward's part of the workspace, which nothing uses between evaluations.
            const bool skip_mix = m->skip_mix_route(W);
            const float* sc = nullptr;
            if (skip_mix && m->cin_total > 1) {
                PackSrc src{};
                src.c0 = 1;
                for (int i = 0; i < 3; ++i)
                    if (chs[i]) { src.ptr[src.n] = srcs[i]; src.ch[src.n] = chs[i]; ++src.n; }
                m->ws_used = 0;
                m->partial = m->wsalloc(sbgm_model::PARTIAL_FLOATS);
                float* x0 = m->partial ? m->wsalloc((size_t)BE * H * W * m->cs_in) : nullptr;
                if (!x0) return 1;
                if (sbgm_launch_pack_input(src, x0, BE, H, W, m->cs_in, st)) return 1;
                ConvParams p{};
                p.x = x0; p.out = skip_Sc(); p.B = BE; p.H = H; p.W = W; p.Cs = m->cs_in; p.Cout = 64;
                p.c_real = m->cin_total == 2 ? 2 : 0;
                if (m->conv(ConvGeom{8, 8, 2, 3}, p, *m->conv1.w, st)) return 1;
                sc = skip_Sc();
            }
            m->set_routes(CALL_SDE_RUN, term, tbrun, BE, skip_mix, sc);
        }
        if (a.tile_origins && draws_noise) {
            SBGM_CHECK(W % 4 == 0 && a.domain_w >= W, "%s: tiled noise needs W %% 4 == 0 and domain_w >= W (W=%d, domain_w=%d)", who, W, a.domain_w);
            nm = NoiseMap{a.tile_origins, H, W / 4, (a.domain_w + 3) / 4};
        }
        if (plan && draws_noise) {
            SBGM_CHECK(per % 4 == 0, "%s: noise rows need H * W %% 4 == 0 (H=%d, W=%d)", who, H, W);
            if (plan->domain_h > 0) {                       // the domain plan rides on the tile map set above (check_plan: origins given)
                SBGM_CHECK(nm.origins != nullptr && plan->domain_h >= H, "%s: a domain noise row over %d rows needs tiles of at most that "
                           "height (H=%d)", who, plan->domain_h, H);
                nm = sbgm_noise_domain_map(nm, plan->rows, plan->domain_h, plan->stride, plan->lags, plan->w);
            } else {
                nm = sbgm_noise_rows_map(plan->rows, plan->stride, plan->lags, plan->w, per);
            }
        }
        saved_ws = m->ws_bytes;
        m->ws_bytes -= keep();       // forward() must not touch the run's slabs
        return 0;
    }
    // One (possibly guided) score evaluation of slab 0 at t_vec() into dst[0 .. n), with guidance through scratch[0 .. 2n): in place for
    // the SDE steps (dst = scratch = the score slab), from a scratch slab into the stage's own for the ODE.
    int evaluate(float* dst, float* scratch, float w) {
        float* xs = slab_at(0);
        if (guided) SBGM_HIP(hipMemcpyAsync(xs + n, xs, n * 4, hipMemcpyDeviceToDevice, st));
        if (m->forward(xs, t_vec(), conds.y, conds.cond, conds.lsm, conds.topo, guided ? scratch : dst, nullptr, BE, H, W, a.bn_train, st)) return 1;
        return guided ? sbgm_launch_cfg_combine(dst, scratch, scratch + n, w, n, st) : 0;
    }
    // ensure_step_graph under k = value-initialised (the padding bytes compare equal) + the kind's own fields + what every kind bakes in
    int capture(StepGraphKey& k, const std::function<int()>& body) {
        k.B = B; k.H = H; k.W = W; k.kind = a.kind; k.guided = guided; k.bn_train = a.bn_train;
        k.y = conds.y; k.cond = conds.cond; k.lsm = conds.lsm; k.topo = conds.topo;
        k.ws = m->ws; k.ws_bytes = saved_ws; k.cfg = a.cfg_scale; k.plan_gen = m->store.plan_gen;
        return m->store.ensure_step_graph(k, guided, st, body);
    }
    int replay_done(int rc) {        // after the last replay; a guided graph goes: its condition copies are freed when the call returns
        if (graphed && m->store.step_exec && hipEventRecord(m->store.ev_replayed, st) != hipSuccess && !rc) { sbgm_set_error("hipEventRecord failed"); rc = 2; }
        if (graphed && guided) m->store.drop_step_graph();
        return rc;
    }
};

// A noise plan keys and mixes the in-kernel draws of independent samples: it is refused, not composed, where the run's noise is decided
// otherwise (injected draws, domain-keyed tiles, a joint run).  The domain plan (domain_h > 0) is the plan OF domain-keyed tiles: it needs
// tile_origins, serves tiled and joint runs, and is not served by the ODE solver (`steps` false).
static int check_plan(const sbgm_model::NoiseRows* p, const sbgm_sampler_args& a, bool joint, const char* who, bool steps = true) {
    if (!p) return 0;
    SBGM_CHECK(p->lags >= 1 && p->lags <= SBGM_NOISE_MAX_LAGS, "%s: noise rows need 1 <= lags <= %d, got %d", who, SBGM_NOISE_MAX_LAGS, p->lags);
    SBGM_CHECK(p->stride >= 1, "%s: noise row stride %d must be >= 1", who, p->stride);
    SBGM_CHECK(p->rows != nullptr, "%s: a noise plan needs its rows table", who);
    SBGM_CHECK(a.noise == nullptr, "%s: noise rows key the in-kernel noise; they cannot be combined with injected noise", who);
    if (p->domain_h > 0) {
        SBGM_CHECK(steps, "%s: a domain noise row is not served by the ODE solver", who);
        SBGM_CHECK(a.tile_origins != nullptr, "%s: a domain noise row needs tile_origins (it is the row of all tiles of one domain)", who);
        return 0;
    }
    SBGM_CHECK(a.tile_origins == nullptr && !joint, "%s: noise rows and tile_origins (tiled or joint runs) exclude each other", who);
    return 0;
}

// The tile table of a run that trusts it (a joint run's ramps, a domain plan's counters: a tile outside the domain would reach into the
// counters of another row), read back once per call (a few bytes; this waits for the stream); `row`: the domain plan's device row, read
// with it and checked against (lags - 1) * stride, or null
static int check_origins(const sbgm_sampler_args& a, int domain_h, const int* row, int lags, int stride, const char* what, hipStream_t st) {
    std::vector<int> org(2 * (size_t)a.B);
    int r = 0;
    SBGM_HIP(hipMemcpyAsync(org.data(), a.tile_origins, org.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    if (row) SBGM_HIP(hipMemcpyAsync(&r, row, sizeof(int), hipMemcpyDeviceToHost, st));
    SBGM_HIP(hipStreamSynchronize(st));
    for (int t = 0; t < a.B; ++t) {
        const int y0 = org[2 * t], x0 = org[2 * t + 1];
        SBGM_CHECK(y0 >= 0 && x0 >= 0 && x0 % 4 == 0 && y0 + a.H <= domain_h && x0 + a.W <= a.domain_w,
                   "sampler: %s tile %d at (%d, %d) of %d x %d does not lie quad-aligned inside the %d x %d domain", what, t, y0, x0, a.H,
                   a.W, domain_h, a.domain_w);
    }
    SBGM_CHECK(!row || (long long)r >= (long long)(lags - 1) * stride, "sampler: the domain noise row %d must be >= (lags - 1) * stride = %lld "
               "(it would reach below row 0)", r, (long long)(lags - 1) * stride);
    return 0;
}

int sbgm_model::sampler(const sbgm_sampler_args& a, hipStream_t caller, const EdmArgs* edm, const HeldArgs* held,
                        const JointArgs* joint, const DpmArgs* dpm, const NoiseRows* plan) {
    if (check_plan(plan, a, joint != nullptr, "sampler")) return 1;
    const bool domain_plan = plan && plan->domain_h > 0;
    SBGM_CHECK(!held || (held->known && held->mask), "sampler: a constrained run needs both known and known_mask");
    if (joint) {
        SBGM_CHECK(a.tile_origins != nullptr, "sampler: a joint run needs tile_origins (its samples are the tiles of one domain)");
        SBGM_CHECK(a.noise == nullptr, "sampler: a joint run draws domain-keyed in-kernel noise; it cannot take injected noise");
        SBGM_CHECK(!a.bn_train, "sampler: a joint run serves eval-mode BatchNorm only (bn_train must be 0)");
        SBGM_CHECK(joint->ramp_len >= 1, "sampler: joint ramp length %d must be >= 1", joint->ramp_len);
        SBGM_CHECK(a.B >= 1 && a.W >= 4 && a.W % 4 == 0, "sampler: a joint run needs B >= 1 and W %% 4 == 0 (B=%d, W=%d)", a.B, a.W);
        SBGM_CHECK(!domain_plan || plan->domain_h == joint->domain_h, "sampler: the domain noise row is over %d rows, the joint run over %d",
                   plan->domain_h, joint->domain_h);
    }
    if (joint || domain_plan) {
        SBGM_CHECK(!domain_plan || (a.B >= 1 && a.W >= 4 && a.W % 4 == 0 && a.domain_w >= a.W), "sampler: a domain noise row needs B >= 1, "
                   "W %% 4 == 0 and domain_w >= W (B=%d, W=%d, domain_w=%d)", a.B, a.W, a.domain_w);
        if (check_origins(a, joint ? joint->domain_h : plan->domain_h, domain_plan ? plan->rows : nullptr, domain_plan ? plan->lags : 1,
                          domain_plan ? plan->stride : 1, joint ? "joint" : "domain-row", caller)) return 1;
    }
    SBGM_CHECK(!(edm && dpm), "sampler: EDM Heun and 2M arguments exclude each other");
    // only sbgm_sampler_run_edm* pass EDM arguments, only sbgm_sampler_run_dpmpp passes 2M arguments
    const StepKind* const kp = step_kind(a.kind, edm != nullptr, dpm != nullptr);
    SBGM_CHECK(kp != nullptr, "sampler: unknown kind %d", a.kind);
    const StepKind& k = *kp;
    const bool heun = edm != nullptr, dpm2m = dpm != nullptr;    // the step body's own branches
    const bool dpm_sde = dpm2m && dpm->eta > 0.f;                // 2M SDE: every step takes a draw
    SBGM_CHECK(a.num_steps >= 2, "sampler: num_steps=%d must be >= 2 (step size = t0 - t1)", a.num_steps);
    SBGM_CHECK(a.out != nullptr, "sampler: out is required");
    SamplerRun run{this, a, caller, "sampler", a.use_graph && !a.noise};
    run.plan = plan;
    if (run.open()) return 1;
    const int B = a.B, N = a.num_steps, BE = run.BE;
    const size_t per = run.per, n = run.n;
    hipStream_t& st = run.st;

    // ---- step table, initial state, hold levels and time rows ------------------------------------------------------------------
    StepStage staged{a, edm, dpm, held != nullptr, k.keeps_rows && a.y == nullptr && env_time_rows(), BE};
    if (store.stage(*this, k, staged, st)) return 1;
    const StepTable& tab = staged.tab;
    const TimeRows& trows = staged.rows;
    run.tbrun = trows.tbrun;
    Hold hold{};
    if (held) {
        hold.known = held->known;
        hold.mask = held->mask;
        hold.z0 = k.hold_draw0 && !dpm_sde ? a.noise : nullptr;        // the deterministic kinds hold with the run's draw 0
        hold.seed = a.seed;
        hold.levels = staged.levels;
    }
    SamplerState* const d_state = store.d_state;
    const StepScalars* sde_tab = static_cast<const StepScalars*>(staged.table);
    const EdmStep* edm_tab = static_cast<const EdmStep*>(staged.table);
    const DpmStep* dpm_tab = static_cast<const DpmStep*>(staged.table);

    if (run.begin()) return 1;
    hold.nm = run.nm;
    const JointMap jm = joint ? JointMap{a.tile_origins, B, a.H, a.W, joint->domain_h, a.domain_w, joint->ramp_len} : JointMap{};
    // slabs: x (the network input), score, x_mean, and for EDM Heun the derivative d; EDM Heun keeps its state x / x_hat in x_mean;
    // 2M keeps its state in the network input and its history D_{i-1} in x_mean
    float *xs = run.slab_at(0), *score = run.slab_at(1), *xmean = run.slab_at(2), *dheun = run.slabs > 3 ? run.slab_at(3) : nullptr;
    float* t_dev = run.t_vec();
    double* sumsq = run.partials();                          // the Langevin corrector's norm partials

    // x0 = randn * marginal_prob_std(1); the Karras kinds: sigma_0 z; into the kind's state slab, copied to the network input
    const float sig = cfg.sigma, ls = logf(sig);
    const float std1 = fmaxf(sqrtf((expf((2.f * 1.0f) * ls) - 1.f) / (2.f * ls)), 1e-5f);
    const float* z = a.noise;
    size_t draw = 0;
    auto next_z = [&]() -> const float* { const float* p = z ? z + draw * n : nullptr; ++draw; return p; };
    float* const state = run.slab_at(k.state_slab);
    if (sbgm_launch_init_noise(state, k.row_sigma ? staged.sigma0 : std1, next_z(), a.seed, d_state, 0, n, st, run.nm, hold)) return 1;
    if (state != xs) SBGM_HIP(hipMemcpyAsync(xs, state, n * 4, hipMemcpyDeviceToDevice, st));
    if (sbgm_launch_fill_t(t_dev, tab.t_first, BE, st)) return 1;
    const float snr_nn = (float)((double)a.snr * std::sqrt((double)per));     // snr * sqrt(prod(x.shape[1:])) (:202-203)

    auto evaluate = [&](float w) { return run.evaluate(score, score, w); };
    const bool churn = heun && edm->s_churn > 0.f;
    // One step of the run's kind; z_ptrs: read the caller's noise draws (eager runs).
    //   EM:  eval -> predictor + advance          PC: eval -> Langevin corrector -> eval -> predictor + advance
    //   EDM: (churn) -> eval -> euler -> eval -> heun + advance; `last` (sigma_N = 0) is Euler only, into `out`
    //   2M:  eval -> update + advance, all N steps alike (the last row of the table makes x_N = D_{N-1})
    auto step = [&](bool z_ptrs, bool last) -> int {
        if (dpm2m) {
            if (evaluate(a.cfg_scale)) return 1;
            return sbgm_launch_dpmpp_2m(xs, nullptr, score, xmean, z_ptrs && dpm_sde ? next_z() : nullptr, dpm_tab, d_state, nullptr, 0, a.seed,
                                        dpm_sde, t_dev, BE, N, n, st, run.nm, hold, jm, trows);
        }
        if (heun) {
            if (churn && sbgm_launch_edm_churn(xmean, xs, z_ptrs ? next_z() : nullptr, edm_tab, d_state, nullptr, 0, a.seed, n, st, run.nm))
                return 1;
            if (evaluate(a.cfg_scale)) return 1;
            if (sbgm_launch_edm_euler(xmean, score, dheun, last ? a.out : xs, edm_tab, d_state, nullptr, t_dev, BE, n, st, hold, jm)) return 1;
            if (last) return 0;
            if (evaluate(a.cfg_scale)) return 1;
            return sbgm_launch_edm_heun(xmean, xs, dheun, score, edm_tab, d_state, nullptr, t_dev, BE, N, n, st, hold, jm);
        }
        if (a.kind == SBGM_SAMPLER_PC) {
            if (evaluate(a.cfg_scale_corrector)) return 1;
            if (sbgm_launch_langevin(xs, score, z_ptrs ? next_z() : nullptr, snr_nn, sumsq, d_state, 0, a.seed, B, per, st, run.nm, hold, jm)) return 1;
        }
        if (evaluate(a.cfg_scale)) return 1;
        return sbgm_launch_em_update(xs, xmean, score, z_ptrs ? next_z() : nullptr, sde_tab, d_state, nullptr, 0, t_dev, a.seed, B,
                                     per, N, st, BE, run.nm, hold, jm, trows);
    };
    // The run: N - tail steps (replays of the captured step, or eager launches), then the kind's `tail` eager last steps, which write
    // `out` themselves; without a tail the result is the kind's result slab, copied to `out`.
    const int tail = k.tail;
    int rc = 0;
    if (run.graphed) {
        StepGraphKey key{};
        key.churn = churn || dpm_sde; key.domain_w = a.domain_w; key.origins = a.tile_origins; key.table = staged.table;
        key.cfg_corr = k.key_corrector ? a.cfg_scale_corrector : 0.f; key.snr_nn = k.key_corrector ? snr_nn : 0.f;
        key.known = hold.known; key.known_mask = hold.mask; key.levels = hold.levels;
        if (joint) { key.joint = 1; key.domain_h = joint->domain_h; key.ramp_len = joint->ramp_len; }
        key.rows = trows.rows; key.tbrun = trows.tbrun;
        if (plan) {                  // the rows' contents are read by every replay, like the conditions'; everything else is baked in
            key.noise_rows = plan->rows; key.noise_stride = plan->stride; key.noise_lags = plan->lags; key.noise_domain_h = plan->domain_h;
            std::copy(plan->w, plan->w + plan->lags, key.noise_w);
        }
        rc = run.capture(key, [&] { return step(false, false); });
        for (int i = 0; i < N - tail && rc == 0; ++i)
            if (hipGraphLaunch(store.step_exec, st) != hipSuccess) { sbgm_set_error("hipGraphLaunch failed at step %d", i); rc = 2; }
    } else {
        for (int i = 0; i < N - tail && rc == 0; ++i) rc = step(z != nullptr, false);
    }
    if (tail && rc == 0) rc = step(z != nullptr, true);
    if ((rc = run.replay_done(rc))) return rc;
    if (!tail) SBGM_HIP(hipMemcpyAsync(a.out, run.slab_at(k.result_slab), n * 4, hipMemcpyDeviceToDevice, st));
    return 0;
}

// rk45_sampler: the adaptive probability-flow ODE solver (ode.hip).  The fourth kind shares the run context above (workspace rule,
// condition handling, cached step graph); what differs is the loop: its length is decided on the device.  One ATTEMPT is
// captured (six stage kernels with their evaluations, the norm, the controller, a 4-byte copy of the done word to pinned memory, the
// commit): a linear chain that depends on nothing that changes between attempts or runs, because t, h, tolerances, flags and counters
// live in the device state block.  The host replays it on the caller's stream and stays at most one attempt ahead of the done word it
// waits for, so the device does not idle on the poll; an attempt that runs after done finds every controller frozen and changes
// nothing.  It sets no route (set_routes).
int sbgm_model::sampler_ode(const sbgm_sampler_args& a, hipStream_t caller, const OdeArgs& o, const NoiseRows* plan) {
    if (check_plan(plan, a, false, "sampler_ode", false)) return 1;
    SBGM_CHECK(!(plan && o.x0), "sampler_ode: noise rows key the start draw; they cannot be combined with a start state x0");
    SBGM_CHECK(a.kind == SBGM_SAMPLER_RK45, "sampler_ode: kind %d is not SBGM_SAMPLER_RK45", a.kind);
    SBGM_CHECK(a.out != nullptr && o.stats_i != nullptr, "sampler_ode: out and stats_i are required");
    SBGM_CHECK(!a.bn_train, "sampler_ode: serves eval-mode BatchNorm only (bn_train must be 0)");
    SBGM_CHECK(o.rtol > 0 && o.atol >= 0 && o.max_steps >= 1, "sampler_ode: need rtol > 0, atol >= 0, max_steps >= 1");
    SBGM_CHECK(o.t0 != o.t1 && std::min(o.t0, o.t1) >= 0.0 && std::max(o.t0, o.t1) <= 1.0, "sampler_ode: t_span (%g, %g) must be two "
               "different times in [0, 1]", o.t0, o.t1);
    SBGM_CHECK(!(a.tile_origins && !o.per_sample), "sampler_ode: tiles need one controller per sample (a shared step would couple them)");
    SamplerRun run{this, a, caller, "sampler_ode", a.use_graph != 0};
    run.plan = plan;
    if (run.open()) return 1;
    const int B = a.B, G = o.per_sample ? B : 1;
    const size_t per = run.per, n = run.n;
    hipStream_t& st = run.st;
    if (!store.h_done) {
        SBGM_HIP(hipHostMalloc(reinterpret_cast<void**>(&store.h_done), 64, hipHostMallocDefault));
        for (hipEvent_t& e : store.ev_poll) SBGM_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }

    if (run.begin(o.x0 == nullptr)) return 1;
    // the 14 slabs: xs | score2 | K[0..6] | y, y | y_new, y_new | state + partials
    float *xs = run.slab_at(0), *score2 = run.slab_at(1), *K = run.slab_at(2), *t_dev = run.t_vec();
    const size_t ks = run.slab / 4;
    double *y = reinterpret_cast<double*>(run.slab_at(9)), *y_new = reinterpret_cast<double*>(run.slab_at(11));
    char* state = reinterpret_cast<char*>(run.slab_at(13));
    const size_t state_bytes = align_up(sbgm_ode_state_bytes(G), 256);
    double* partials = reinterpret_cast<double*>(state + state_bytes);
    SBGM_CHECK(state_bytes + sbgm_ode_partials_bytes(B, per) <= run.slab, "sampler_ode: %d x %d samples are too small for the solver's state slab", a.H, a.W);

    // start: the caller's state, or marginal_prob_std(t0) * draw 0 of the run's Philox stream (domain-keyed on tiles)
    if (sbgm_launch_ode_init(state, G, o.t0, o.t1, o.rtol, o.atol, cfg.sigma, o.max_steps, st)) return 1;
    if (o.x0) {
        if (sbgm_launch_ode_load(y, o.x0, n, st)) return 1;
    } else {
        const float ls = logf(cfg.sigma), t0f = (float)o.t0;
        const float std0 = fmaxf(sqrtf((expf((2.f * t0f) * ls) - 1.f) / (2.f * ls)), 1e-5f);
        if (sbgm_launch_init_noise(xs, std0, a.noise, a.seed, nullptr, 0, n, st, run.nm)) return 1;
        if (sbgm_launch_ode_load(y, xs, n, st)) return 1;
    }

    auto evaluate = [&](float* dst) { return run.evaluate(dst, score2, a.cfg_scale); };
    auto stage = [&](int phase) -> int {
        return sbgm_launch_ode_stage(state, phase, y, y_new, K, ks, xs, t_dev, run.guided ? 2 : 1, B, per, o.per_sample, st);
    };
    auto control = [&](int what) -> int {
        if (sbgm_launch_ode_control(state, what, y, y_new, K, ks, partials, B, per, o.per_sample, st)) return 1;
        SBGM_HIP(hipMemcpyAsync(store.h_done, state + offsetof(OdeHeader, done), 4, hipMemcpyDeviceToHost, st));
        return 0;
    };
    auto attempt = [&]() -> int {
        for (int s = 1; s <= 6; ++s)
            if (stage(s) || evaluate(K + (size_t)s * ks)) return 1;
        if (control(2)) return 1;
        return sbgm_launch_ode_commit(state, y, y_new, K, ks, B, per, o.per_sample, st);
    };

    long long enqueued = 0;
    // select_initial_step: f0, the two norms, f1 at t0 + h0, the third norm; then the first attempt is prepared
    int rc = stage(SBGM_ODE_PHASE_F0) || evaluate(K) || control(0) || stage(SBGM_ODE_PHASE_F1) || evaluate(K + ks) || control(1);
    if (rc == 0 && (hipEventRecord(store.ev_poll[0], st) != hipSuccess || hipEventSynchronize(store.ev_poll[0]) != hipSuccess)) {
        sbgm_set_error("sampler_ode: waiting for the initial step failed: %s", hipGetErrorString(hipGetLastError()));
        rc = 2;
    }
    volatile int* done = store.h_done;
    if (rc == 0 && !*done) {
        if (run.graphed) {
            StepGraphKey key{};
            key.ode_norm = o.per_sample;
            rc = run.capture(key, attempt);
        }
        auto launch = [&]() -> int {
            if (run.graphed) {
                if (hipGraphLaunch(store.step_exec, st) != hipSuccess) { sbgm_set_error("hipGraphLaunch failed at attempt %lld", enqueued); return 2; }
            } else if (attempt()) {
                return 1;
            }
            if (hipEventRecord(store.ev_poll[enqueued & 1], st) != hipSuccess) { sbgm_set_error("hipEventRecord failed"); return 2; }
            ++enqueued;
            return 0;
        };
        // every controller stops within max_steps attempts, so max_steps + 1 enqueued attempts always reach done
        const long long cap = o.max_steps + 1;
        for (long long k = 0; rc == 0; ++k) {                    // k: the attempt whose done word the host waits for
            while (rc == 0 && enqueued <= k + 1 && enqueued < cap) rc = launch();     // at most one attempt ahead of it
            if (rc) break;
            if (hipEventSynchronize(store.ev_poll[k & 1]) != hipSuccess) { sbgm_set_error("sampler_ode: waiting for attempt %lld failed", k); rc = 2; }
            if (rc || *done) break;
            if (k + 1 >= cap) { sbgm_set_error("sampler_ode: %lld attempts did not finish the run", cap); rc = 2; }
        }
    }
    if ((rc = run.replay_done(rc))) return rc;
    if (sbgm_launch_ode_store(a.out, y, n, st)) return 1;
    if (sbgm_ode_read_state(state, G, o.stats_i, o.stats_d, st)) return 1;       // synchronises: the run is complete on return
    o.stats_i[4 * G] = enqueued - o.stats_i[4 * G + 1];                            // surplus attempts: enqueued, found nothing to do
    o.stats_i[4 * G + 1] = enqueued;
    return 0;
}

static int edm_args_check(const sbgm_sampler_args* a, const sbgm_model::EdmArgs& e) {
    SBGM_CHECK(a->kind == SBGM_SAMPLER_EDM_HEUN, "sampler_run_edm: kind %d is not SBGM_SAMPLER_EDM_HEUN", a->kind);
    SBGM_CHECK(!a->bn_train, "sampler_run_edm: serves eval-mode BatchNorm only (bn_train must be 0)");
    SBGM_CHECK(e.rho > 0.f && e.s_churn >= 0.f && e.s_noise >= 0.f, "sampler_run_edm: need rho > 0, s_churn >= 0, s_noise >= 0");
    SBGM_CHECK(!(e.sigma_min > 0.f && e.sigma_max > 0.f && e.sigma_min >= e.sigma_max), "sampler_run_edm: sigma_min %g >= sigma_max %g",
               e.sigma_min, e.sigma_max);
    return 0;
}
static int dpm_args_check(const sbgm_sampler_args* a, const sbgm_model::DpmArgs& d) {
    SBGM_CHECK(a->kind == SBGM_SAMPLER_DPMPP_2M, "sampler_run_dpmpp: kind %d is not SBGM_SAMPLER_DPMPP_2M", a->kind);
    SBGM_CHECK(!a->bn_train, "sampler_run_dpmpp: serves eval-mode BatchNorm only (bn_train must be 0)");
    SBGM_CHECK(d.rho > 0.f && d.eta >= 0.f && d.s_noise >= 0.f, "sampler_run_dpmpp: need rho > 0, eta >= 0, s_noise >= 0");
    SBGM_CHECK(!(d.sigma_min > 0.f && d.sigma_max > 0.f && d.sigma_min >= d.sigma_max), "sampler_run_dpmpp: sigma_min %g >= sigma_max %g",
               d.sigma_min, d.sigma_max);
    return 0;
}

// What the seven step-sampler entry points share: the same sbgm_model::sampler with the optional parts they pass.  `who`: the entry
// point in the messages; `edm` / `dpm`: the kind's scalars or null; `need_known`: a held driver (known and known_mask required; every
// other driver takes both or neither, the plain ones neither); `joint`: the B tiles are one domain of domain_h rows.
static int run_steps(sbgm_model* m, const sbgm_sampler_args* a, const char* who, const sbgm_model::EdmArgs* edm, const sbgm_model::DpmArgs* dpm,
                     bool need_known, const float* known, const float* known_mask, bool joint, int domain_h, int ramp_len, void* stream) {
    SBGM_CHECK(a, "%s: null args", who);
    SBGM_CHECK(!need_known || (known && known_mask), "%s: known and known_mask are required", who);
    if (dpm && dpm_args_check(a, *dpm)) return 1;            // 2M names its scalars before its tensors
    SBGM_CHECK((known == nullptr) == (known_mask == nullptr), "%s: known and known_mask must be given together", who);
    if (edm && edm_args_check(a, *edm)) return 1;
    const sbgm_model::HeldArgs h{known, known_mask};
    const sbgm_model::JointArgs j{domain_h, ramp_len};
    return m->sampler(*a, (hipStream_t)stream, edm, known ? &h : nullptr, joint ? &j : nullptr, dpm, m->noise_rows.rows ? &m->noise_rows : nullptr);
}

extern "C" {

// The noise plan of the handle's sampler runs: copied into the handle (the rows table itself stays the caller's), used by every entry
// point below until cleared.
int sbgm_sampler_set_noise_rows(sbgm_model* m, const int32_t* rows, int stride, const float* weights, int lags) {
    SBGM_CHECK(m, "sampler_set_noise_rows: null model");
    if (rows == nullptr) {
        SBGM_CHECK(lags <= 1, "sampler_set_noise_rows: %d lags need a rows table (NULL rows clear the plan)", lags);
        m->noise_rows = sbgm_model::NoiseRows{};
        return 0;
    }
    SBGM_CHECK(lags >= 1 && lags <= SBGM_NOISE_MAX_LAGS, "sampler_set_noise_rows: lags=%d must be in 1..%d", lags, SBGM_NOISE_MAX_LAGS);
    SBGM_CHECK(stride >= 1, "sampler_set_noise_rows: stride=%d must be >= 1", stride);
    SBGM_CHECK(weights != nullptr, "sampler_set_noise_rows: weights are required");
    SBGM_CHECK(m->noise_rows.domain_h == 0, "sampler_set_noise_rows: the handle holds a domain noise row; the two plans exclude each other "
               "(clear it with sbgm_sampler_set_noise_domain_row(m, NULL, ...))");
    sbgm_model::NoiseRows p;
    p.rows = rows; p.stride = stride; p.lags = lags;
    std::copy(weights, weights + lags, p.w);
    m->noise_rows = p;
    return 0;
}

// The domain noise plan of the handle's tiled sampler runs: ONE device row for all tiles of a domain of domain_h rows (the row itself
// stays the caller's and is read by the kernels, so a new value at the same address replays the same captured step).
int sbgm_sampler_set_noise_domain_row(sbgm_model* m, const int32_t* row_dev, int domain_h, int stride, const float* weights, int lags) {
    SBGM_CHECK(m, "sampler_set_noise_domain_row: null model");
    if (row_dev == nullptr) {
        SBGM_CHECK(lags <= 1, "sampler_set_noise_domain_row: %d lags need a row (a NULL row clears the plan)", lags);
        m->noise_rows = sbgm_model::NoiseRows{};
        return 0;
    }
    SBGM_CHECK(lags >= 1 && lags <= SBGM_NOISE_MAX_LAGS, "sampler_set_noise_domain_row: lags=%d must be in 1..%d", lags, SBGM_NOISE_MAX_LAGS);
    SBGM_CHECK(stride >= 1, "sampler_set_noise_domain_row: stride=%d must be >= 1", stride);
    SBGM_CHECK(domain_h >= 1, "sampler_set_noise_domain_row: domain_h=%d must be >= 1", domain_h);
    SBGM_CHECK(weights != nullptr, "sampler_set_noise_domain_row: weights are required");
    SBGM_CHECK(m->noise_rows.rows == nullptr || m->noise_rows.domain_h > 0, "sampler_set_noise_domain_row: the handle holds a rows plan; the "
               "two plans exclude each other (clear it with sbgm_sampler_set_noise_rows(m, NULL, ...))");
    sbgm_model::NoiseRows p;
    p.rows = row_dev; p.stride = stride; p.lags = lags; p.domain_h = domain_h;
    std::copy(weights, weights + lags, p.w);
    m->noise_rows = p;
    return 0;
}

int sbgm_sampler_run(sbgm_model* m, const sbgm_sampler_args* a, void* stream) {
    return run_steps(m, a, "sampler_run", nullptr, nullptr, false, nullptr, nullptr, false, 0, 0, stream);
}

int sbgm_sampler_run_edm(sbgm_model* m, const sbgm_sampler_args* a, float sigma_min, float sigma_max, float rho, float s_churn,
                         float s_tmin, float s_tmax, float s_noise, void* stream) {
    const sbgm_model::EdmArgs e{sigma_min, sigma_max, rho, s_churn, s_tmin, s_tmax, s_noise};
    return run_steps(m, a, "sampler_run_edm", &e, nullptr, false, nullptr, nullptr, false, 0, 0, stream);
}

// The two drivers above with a constraint (constrained sampling): the held kernels.
int sbgm_sampler_run_held(sbgm_model* m, const sbgm_sampler_args* a, const float* known, const float* known_mask, void* stream) {
    return run_steps(m, a, "sampler_run_held", nullptr, nullptr, true, known, known_mask, false, 0, 0, stream);
}

int sbgm_sampler_run_edm_held(sbgm_model* m, const sbgm_sampler_args* a, float sigma_min, float sigma_max, float rho, float s_churn,
                              float s_tmin, float s_tmax, float s_noise, const float* known, const float* known_mask, void* stream) {
    const sbgm_model::EdmArgs e{sigma_min, sigma_max, rho, s_churn, s_tmin, s_tmax, s_noise};
    return run_steps(m, a, "sampler_run_edm_held", &e, nullptr, true, known, known_mask, false, 0, 0, stream);
}

// The drivers above as ONE diffusion over the domain (joint tiled sampling): the joint kernels; known / known_mask may
// both be NULL.
int sbgm_sampler_run_joint(sbgm_model* m, const sbgm_sampler_args* a, int domain_h, int ramp_len, const float* known,
                           const float* known_mask, void* stream) {
    return run_steps(m, a, "sampler_run_joint", nullptr, nullptr, false, known, known_mask, true, domain_h, ramp_len, stream);
}

int sbgm_sampler_run_edm_joint(sbgm_model* m, const sbgm_sampler_args* a, float sigma_min, float sigma_max, float rho, float s_churn,
                               float s_tmin, float s_tmax, float s_noise, int domain_h, int ramp_len, const float* known,
                               const float* known_mask, void* stream) {
    const sbgm_model::EdmArgs e{sigma_min, sigma_max, rho, s_churn, s_tmin, s_tmax, s_noise};
    return run_steps(m, a, "sampler_run_edm_joint", &e, nullptr, false, known, known_mask, true, domain_h, ramp_len, stream);
}

// DPM-Solver++(2M) / 2M SDE with its optional parts as arguments: the dpmpp_2m kernels.
int sbgm_sampler_run_dpmpp(sbgm_model* m, const sbgm_sampler_args* a, float sigma_min, float sigma_max, float rho, float eta, float s_noise,
                           const float* known, const float* known_mask, int domain_h, int ramp_len, void* stream) {
    const sbgm_model::DpmArgs d{sigma_min, sigma_max, rho, eta, s_noise};
    return run_steps(m, a, "sampler_run_dpmpp", nullptr, &d, false, known, known_mask, domain_h || ramp_len, domain_h, ramp_len, stream);
}

int sbgm_sampler_run_ode(sbgm_model* m, const sbgm_sampler_args* a, double t0, double t1, double rtol, double atol, int per_sample,
                         int64_t max_steps, const float* x0, int64_t* stats_i, double* stats_d, void* stream) {
    SBGM_CHECK(a, "sampler_run_ode: null args");
    const sbgm_model::OdeArgs o{t0, t1, rtol, atol, per_sample != 0, (long long)max_steps, x0, stats_i, stats_d};
    return m->sampler_ode(*a, (hipStream_t)stream, o, m->noise_rows.rows ? &m->noise_rows : nullptr);
}

}  // extern "C"
