// pedn_metrics.hpp -- the reference's evaluation metrics (rl/rl_utils.py:770-1512) for every replica on the device: pedn_metrics_begin /
// pedn_metrics_accumulate / pedn_metrics_read of include/pedn.h.  Like every subsystem header it is included behind pedn_host.hpp (it
// uses the engine's handle and the core's ordering services); the core calls metrics_free, nothing here is called by a step.
//
// metrics_accumulate_kernel: one wave per (link, 64 replicas), lane = replica.  Each lane walks the rows of its window in order and adds
// into its own f64 accumulators [MA_K][L][RS]: the three f32 fields are read once each, as coalesced 256-byte row segments, and nothing
// else but the link's parameters.  No atomics and no cross-lane sums, so a (link, replica) total is the same serial sum whatever the grid,
// the batch size or the split of the rows into consecutive windows.
// metrics_finalize_kernel: one lane per replica folds the accumulators over the links in link order and adds the row-T and demand terms
// serially in the reference's order.
//
// Compiled with -ffp-contract=off like the rest: every term is the reference's expression evaluated in binary64.

enum { MA_S_TT = 0, MA_C_TT, MA_S_DELAY, MA_S_PTD, MA_S_PT, MA_C_ROWS, MA_S_AREA, MA_C_CONG, MA_S_EXC, MA_S_D, MA_C_D, MA_K };
enum { MF_ORIGIN = 1, MF_DEST = 2, MF_ODPATH = 4 };

struct MetricsState {
  double* acc = nullptr;        // [MA_K][L][RS] (allocated once, in the engine's allocation list)
  void* tables = nullptr;       // link flags, origin rows / lengths, agent pointers / links, outputs (owned, freed by metrics_free)
  const int32_t *flags = nullptr, *orow = nullptr, *olen = nullptr, *aptr = nullptr, *alinks = nullptr;
  double *out = nullptr, *aout_links = nullptr, *aout = nullptr;
  int n_orig = 0, n_agents = 0, n_alinks = 0;
  double unit_time = 1.0;
  int next = 0;      // first row the next window may start at
  int covered = 0;   // rows folded in so far
  bool ready = false;
};

static void metrics_free(pedn_sim* s) {
  if (!s->metrics) return;
  if (s->metrics->tables) hipFree(s->metrics->tables);
  delete s->metrics;
  s->metrics = nullptr;
}

__global__ __launch_bounds__(256) void metrics_accumulate_kernel(const float* __restrict__ tt, const float* __restrict__ np_,
                                                                 const float* __restrict__ dk, int m_tt, int m_n, int m_k,
                                                                 const LinkP* __restrict__ lp, const LinkPR* __restrict__ prm, int pr,
                                                                 double* __restrict__ acc, int L, int RS, int t0, int t1, int hi,
                                                                 double ut) {
  const int nrg = RS >> 6;
  const int w = (int)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (w >= L * nrg) return;
  const int l = w / nrg;
  const int r = (w - l * nrg) * 64 + (int)(threadIdx.x & 63);
  const size_t LR = (size_t)L * RS, me = (size_t)l * RS + r;
  const LinkP& P = lp[l];
  const double length = P.length, width = P.width;
  double kc = P.kc, vf = P.vf;
  if (pr) {
    const LinkPR q = prm[me];
    kc = q.kc;
    vf = q.vf;
  }
  const double area_time = (length * width) * ut;      // rl_utils.py:1471,1484
  const double fftt = length / vf;                      // :1027
  double a[MA_K];
#pragma unroll
  for (int k = 0; k < MA_K; ++k) a[k] = acc[k * LR + me];
  // one row of the reference's loops, widened to f64 (json holds the f32 values as Python floats)
  auto row = [&](float ttf, float nf, float df) {
    const double x = ttf, n = nf, d = df;
    const bool vt = x >= 0;                                            // :944 valid travel time
    a[MA_S_TT] += vt ? x : 0.0;
    a[MA_C_TT] += vt ? 1.0 : 0.0;
    const bool dl = !(x <= 0);                                         // :1045 (NaN is not skipped there)
    double f = 1 - fftt / x;                                           // :1050 delay_fraction = max(0, ...)
    f = f > 0 ? f : 0.0;
    a[MA_S_DELAY] += dl ? n * f * ut : 0.0;                            // :1051 num_peds * delay_fraction * unit_time
    a[MA_S_PTD] += dl ? n * ut : 0.0;                                  // :1054
    a[MA_S_PT] += n >= 0 ? n * ut : 0.0;                               // :1136-1137
    const bool vc = !(d < 0);                                          // :1477
    a[MA_C_ROWS] += vc ? 1.0 : 0.0;
    a[MA_S_AREA] += vc ? area_time : 0.0;
    const bool cg = vc && d > kc;                                      // :1490
    a[MA_C_CONG] += cg ? 1.0 : 0.0;
    a[MA_S_EXC] += cg ? (d - kc) * area_time : 0.0;                    // :1494-1495
    const bool vd = d >= 0;                                            // :1385 (agent-local densities)
    a[MA_S_D] += vd ? d : 0.0;
    a[MA_C_D] += vd ? 1.0 : 0.0;
  };
  const int tl = t1 < hi + 1 ? t1 : hi + 1;   // rows [t0, tl) are read, rows above `hi` read as zero
  int t = t0;
  for (; t + 8 <= tl; t += 8) {   // eight rows of loads in flight before the first is used
    float x[8], n[8], d[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      x[j] = tt[((size_t)((t + j) & m_tt) * L + l) * RS + r];
      n[j] = np_[((size_t)((t + j) & m_n) * L + l) * RS + r];
      d[j] = dk[((size_t)((t + j) & m_k) * L + l) * RS + r];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) row(x[j], n[j], d[j]);
  }
  for (; t < tl; ++t)
    row(tt[((size_t)(t & m_tt) * L + l) * RS + r], np_[((size_t)(t & m_n) * L + l) * RS + r], dk[((size_t)(t & m_k) * L + l) * RS + r]);
  for (t = t0 > tl ? t0 : tl; t < t1; ++t) row(0.0f, 0.0f, 0.0f);
#pragma unroll
  for (int k = 0; k < MA_K; ++k) acc[k * LR + me] = a[k];
}

__global__ __launch_bounds__(256) void metrics_finalize_kernel(const double* __restrict__ acc, const double* __restrict__ ci,
                                                               const double* __restrict__ co, int m_ci, int m_co, int rowT,
                                                               const double* __restrict__ demand, const LinkP* __restrict__ lp,
                                                               const LinkPR* __restrict__ prm, int pr, const int32_t* __restrict__ flags,
                                                               const int32_t* __restrict__ orow, const int32_t* __restrict__ olen,
                                                               int n_orig, const int32_t* __restrict__ aptr,
                                                               const int32_t* __restrict__ alinks, int n_agents, double* __restrict__ out,
                                                               double* __restrict__ aout_links, double* __restrict__ aout, int L,
                                                               int Lall, int T1, int RS, int R, double ut, double uncovered) {
  const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (r >= R) return;
  const size_t LR = (size_t)L * RS;
  const int T = T1 - 1;
  // per (link, replica) totals with the rows no window covered counted as zero rows
  auto total = [&](int l, int k) { return acc[k * LR + (size_t)l * RS + r]; };
  double tt_sum = 0.0, delay = 0.0, pt_delay = 0.0, pt = 0.0, cong = 0.0, area = 0.0, inflow = 0.0, outflow = 0.0;
  double n_tt = 0, n_delay = 0, n_orig_links = 0, n_dest_links = 0, cong_rows = 0, rows = 0;
  for (int l = 0; l < L; ++l) {
    const LinkP& P = lp[l];
    double kc = P.kc, kj = P.kj, vf = P.vf;
    if (pr) {
      const LinkPR q = prm[(size_t)l * RS + r];
      kc = q.kc; kj = q.kj; vf = q.vf;
    }
    const int f = flags[l];
    const double area_time = (P.length * P.width) * ut;
    // a row no window covered reads 0: a valid travel time, density and person count, no delay; congested only if 0 > k_critical
    const bool zc = 0.0 > kc;
    if (f & MF_ODPATH) {                                               // :933-948 mean over the link's valid rows, then over links
      const double c = total(l, MA_C_TT) + uncovered;
      if (c > 0) {
        tt_sum += total(l, MA_S_TT) / c;
        n_tt += 1;
      }
    }
    if (!(vf <= 0)) {                                                  // :1023 links with free_flow_speed <= 0 are skipped
      delay += total(l, MA_S_DELAY);
      pt_delay += total(l, MA_S_PTD);
      n_delay += 1;
    }
    pt += total(l, MA_S_PT);
    if (!(kj <= 0)) {                                                  // :1473
      cong += total(l, MA_S_EXC) + (zc ? uncovered * ((0.0 - kc) * area_time) : 0.0);
      area += total(l, MA_S_AREA) + uncovered * area_time;
      cong_rows += total(l, MA_C_CONG) + (zc ? uncovered : 0.0);
      rows += total(l, MA_C_ROWS) + uncovered;
    }
    if (f & MF_ORIGIN) {                                               // :1143-1156, :1236-1247: cumulative_inflow[-1]
      inflow += rowT >= 0 ? ci[((size_t)(rowT & m_ci) * Lall + l) * RS + r] : 0.0;
      n_orig_links += 1;
    }
    if (f & MF_DEST) {                                                 // :843-859, :1255-1267: cumulative_outflow[-1]
      outflow += rowT >= 0 ? co[((size_t)(rowT & m_co) * Lall + l) * RS + r] : 0.0;
      n_dest_links += 1;
    }
  }
  double demand_total = 0.0;                                           // :830-836: sum(demand) per origin, in origin_nodes order
  for (int o = 0; o < n_orig; ++o) {
    if (orow[o] < 0 || olen[o] <= 0) continue;
    double sd = 0.0;
    const int n = olen[o] < T1 ? olen[o] : T1;
    for (int t = 0; t < n; ++t) sd += demand[((size_t)orow[o] * T1 + t) * RS + r];
    demand_total += sd;
  }
  (void)T;
  double* o = out + (size_t)r * PEDN_N_METRICS;
  o[PEDN_M_THROUGHPUT] = demand_total > 0 ? outflow / demand_total : 0.0;
  o[PEDN_M_COMPLETED_DEMAND] = outflow;
  o[PEDN_M_TOTAL_DEMAND] = demand_total;
  o[PEDN_M_AVG_TRAVEL_TIME] = n_tt > 0 ? tt_sum / n_tt : 0.0;
  o[PEDN_M_TT_NUM_LINKS] = n_tt;
  o[PEDN_M_TOTAL_DELAY] = delay;
  o[PEDN_M_DELAY_INTENSITY] = pt_delay > 0 ? delay / pt_delay : 0.0;
  o[PEDN_M_DELAY_PERSON_TIME] = pt_delay;
  o[PEDN_M_DELAY_NUM_LINKS] = n_delay;
  o[PEDN_M_AVG_TIME_SPENT] = inflow > 0 ? pt / inflow : 0.0;
  o[PEDN_M_PERSON_TIME] = pt;
  o[PEDN_M_TOTAL_TRIPS] = inflow;
  o[PEDN_M_NUM_ORIGIN_LINKS] = n_orig_links;
  o[PEDN_M_SERVED_RATE] = inflow > 0 ? outflow / inflow : 0.0;
  o[PEDN_M_TOTAL_INFLOW] = inflow;
  o[PEDN_M_TOTAL_OUTFLOW] = outflow;
  o[PEDN_M_NUM_DEST_LINKS] = n_dest_links;
  o[PEDN_M_CONGESTION_TIME] = cong;
  o[PEDN_M_AVG_CONGESTION_DENSITY] = area > 0 ? cong / area : 0.0;
  o[PEDN_M_CONGESTION_FRACTION] = area > 0 && rows > 0 ? cong_rows / rows : 0.0;
  o[PEDN_M_TOTAL_AREA_TIME] = area;
  o[PEDN_M_CONGESTED_ROWS] = cong_rows;
  o[PEDN_M_COUNTED_ROWS] = rows;
  // agent-local metrics (:1343-1409): mean density of each of the agent's links, then the mean over those links
  if (!aout_links && !aout) return;
  const double qnan = __builtin_nan("");
  for (int ag = 0; ag < n_agents; ++ag) {
    double sd = 0.0, sn = 0.0, nl = 0;
    for (int j = aptr[ag]; j < aptr[ag + 1]; ++j) {
      const int l = alinks[j];
      const double kj = pr ? prm[(size_t)l * RS + r].kj : lp[l].kj;
      const double c = total(l, MA_C_D) + uncovered;
      double m = qnan, mn = qnan;
      if (c > 0) {
        m = total(l, MA_S_D) / c;
        mn = m / kj;
        sd += m;
        sn += mn;
        nl += 1;
      }
      if (aout_links) {
        aout_links[((size_t)r * aptr[n_agents] + j) * 2] = m;
        aout_links[((size_t)r * aptr[n_agents] + j) * 2 + 1] = mn;
      }
    }
    if (aout) {
      double* a = aout + ((size_t)r * n_agents + ag) * 3;
      a[0] = nl > 0 ? sd / nl : 0.0;
      a[1] = nl > 0 ? sn / nl : 0.0;
      a[2] = nl;
    }
  }
}

extern "C" {

int pedn_metrics_begin(pedn_sim* s, const int32_t* link_flags, const int32_t* origin_rows, const int32_t* origin_len, int32_t n_origins,
                       const int32_t* agent_ptr, const int32_t* agent_links, int32_t n_agents, double unit_time) {
  if (!s || !link_flags) return fail(s, PEDN_E_ARG, "null argument");
  if (n_origins < 0 || n_agents < 0 || (n_origins && (!origin_rows || !origin_len)) || (n_agents && (!agent_ptr || !agent_links)))
    return fail(s, PEDN_E_ARG, "null argument");
  const DevView& v = s->v;
  if (n_agents && (agent_ptr[0] != 0)) return fail(s, PEDN_E_ARG, "agent_ptr must start at 0");
  for (int a = 0; a < n_agents; ++a)
    if (agent_ptr[a + 1] < agent_ptr[a]) return fail(s, PEDN_E_ARG, "agent_ptr must not decrease");
  const int n_alinks = n_agents ? agent_ptr[n_agents] : 0;
  for (int j = 0; j < n_alinks; ++j)
    if (agent_links[j] < 0 || agent_links[j] >= v.L) return fail(s, PEDN_E_ARG, "agent link out of range");
  for (int o = 0; o < n_origins; ++o)
    if (origin_rows[o] >= s->n_demand || origin_rows[o] < -1) return fail(s, PEDN_E_ARG, "origin demand row out of range");
  HIP_TRY(s, hipSetDevice(s->device));
  pending_links_first(s);
  if (!s->metrics) s->metrics = new MetricsState();
  MetricsState& m = *s->metrics;
  if (!m.acc) {
    const int rc = dalloc(s, (size_t)MA_K * v.L * v.RS, &m.acc);
    if (rc != PEDN_OK) return rc;
  }
  HIP_TRY(s, hipStreamSynchronize(s->stream));   // the previous set-up's tables may still be read by an earlier launch
  if (m.tables) {
    hipFree(m.tables);
    m.tables = nullptr;
  }
  m.ready = false;
  // one allocation: int32 tables first, then the f64 outputs at an 8-byte boundary
  std::vector<int32_t> h;
  h.insert(h.end(), link_flags, link_flags + v.L);
  h.insert(h.end(), origin_rows, origin_rows + n_origins);
  h.insert(h.end(), origin_len, origin_len + n_origins);
  if (n_agents) h.insert(h.end(), agent_ptr, agent_ptr + n_agents + 1);
  else h.push_back(0);
  h.insert(h.end(), agent_links, agent_links + n_alinks);
  if (h.size() & 1) h.push_back(0);
  const size_t n_out = (size_t)v.R * (PEDN_N_METRICS + 2 * n_alinks + 3 * n_agents);
  const size_t bytes = h.size() * 4 + n_out * 8;
  HIP_TRY(s, hipMalloc(&m.tables, bytes));
  HIP_TRY(s, hipMemcpy(m.tables, h.data(), h.size() * 4, hipMemcpyHostToDevice));
  const int32_t* p = (const int32_t*)m.tables;
  m.flags = p; p += v.L;
  m.orow = p; p += n_origins;
  m.olen = p; p += n_origins;
  m.aptr = p; p += n_agents + 1;
  m.alinks = p;
  m.out = (double*)((char*)m.tables + h.size() * 4);
  m.aout_links = m.out + (size_t)v.R * PEDN_N_METRICS;
  m.aout = m.aout_links + (size_t)v.R * 2 * n_alinks;
  m.n_orig = n_origins; m.n_agents = n_agents; m.n_alinks = n_alinks;
  m.unit_time = unit_time;
  m.next = 0;
  m.covered = 0;
  HIP_TRY(s, hipMemsetAsync(m.acc, 0, (size_t)MA_K * v.L * v.RS * sizeof(double), s->stream));
  m.ready = true;
  return PEDN_OK;
}

// highest row of a history field that holds what pedn_read would return for it (rows above read as zero); the ring check of pedn_read
static int metrics_hi(const pedn_sim* s) {
  int hi = std::min(s->marks.valid_hi, s->v.T1 - 1);
  if (s->v.hist) hi = std::min(hi, std::max(s->marks.last_t, 0));   // a ring row above the newest step holds an older time index
  return hi;
}

int pedn_metrics_accumulate(pedn_sim* s, int32_t t0, int32_t t1) {
  if (!s) return fail(nullptr, PEDN_E_ARG, "null handle");
  if (!s->metrics || !s->metrics->ready) return fail(s, PEDN_E_ARG, "pedn_metrics_begin has not been called");
  MetricsState& m = *s->metrics;
  const DevView& v = s->v;
  if (t0 < 0 || t1 > v.T1 || t0 > t1) return fail(s, PEDN_E_ARG, "metrics window out of bounds");
  if (t0 < m.next) return fail(s, PEDN_E_ARG, "metrics windows must increase and must not overlap (next row " + std::to_string(m.next) + ")");
  if (t0 == t1) return PEDN_OK;
  HIP_TRY(s, hipSetDevice(s->device));
  pending_links_first(s);   // (also ends a clocked section, so that last_t is the host's again)
  const int hi = metrics_hi(s);
  const int newest = std::max(s->marks.last_t, 0);
  for (int g : {G_TT, G_N, G_K}) {
    const int rows = s->rows32[g];
    if (rows < v.T1 && t0 < std::min(t1, hi + 1) && t0 <= newest - rows)
      return fail(s, PEDN_E_ARG, "time index outside the field's ring (recent-history mode keeps the last " + std::to_string(rows) +
                                 " entries of this field; the newest is " + std::to_string(newest) + ")");
  }
  const unsigned waves = (unsigned)v.L * (unsigned)(v.RS / 64);
  if (waves)
    hipLaunchKernelGGL(metrics_accumulate_kernel, dim3((waves + 3) / 4), dim3(256), 0, s->stream, (const float*)v.f32[G_TT],
                       (const float*)v.f32[G_N], (const float*)v.f32[G_K], v.m32[G_TT], v.m32[G_N], v.m32[G_K], v.lp,
                       (const LinkPR*)v.prm, v.pr, m.acc, v.L, v.RS, t0, t1, hi, m.unit_time);
  HIP_TRY(s, hipGetLastError());
  m.next = t1;
  m.covered += t1 - t0;
  return PEDN_OK;
}

int pedn_metrics_read(pedn_sim* s, double* out, double* agent_links, double* agents) {
  if (!s || !out) return fail(s, PEDN_E_ARG, "null argument");
  if (!s->metrics || !s->metrics->ready) return fail(s, PEDN_E_ARG, "pedn_metrics_begin has not been called");
  MetricsState& m = *s->metrics;
  const DevView& v = s->v;
  HIP_TRY(s, hipSetDevice(s->device));
  pending_links_first(s);
  const int T = v.T1 - 1;
  const int rowT = T <= metrics_hi(s) ? T : -1;   // cumulative flows of row T: zero until a step has written them
  const bool with_agents = m.n_agents > 0 && (agent_links || agents);
  hipLaunchKernelGGL(metrics_finalize_kernel, dim3((unsigned)((v.R + 255) / 256)), dim3(256), 0, s->stream, (const double*)m.acc,
                     (const double*)v.f64[F_CI], (const double*)v.f64[F_CO], v.m64[F_CI], v.m64[F_CO], rowT, (const double*)v.demand,
                     v.lp, (const LinkPR*)v.prm, v.pr, m.flags, m.orow, m.olen, m.n_orig, m.aptr, m.alinks, m.n_agents, m.out,
                     with_agents ? m.aout_links : nullptr, with_agents ? m.aout : nullptr, v.L, v.Lall, v.T1, v.RS, v.R, m.unit_time,
                     (double)(v.T1 - m.covered));
  HIP_TRY(s, hipGetLastError());
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  HIP_TRY(s, hipMemcpy(out, m.out, (size_t)v.R * PEDN_N_METRICS * sizeof(double), hipMemcpyDeviceToHost));
  if (with_agents && agent_links)
    HIP_TRY(s, hipMemcpy(agent_links, m.aout_links, (size_t)v.R * 2 * m.n_alinks * sizeof(double), hipMemcpyDeviceToHost));
  if (with_agents && agents)
    HIP_TRY(s, hipMemcpy(agents, m.aout, (size_t)v.R * 3 * m.n_agents * sizeof(double), hipMemcpyDeviceToHost));
  return PEDN_OK;
}

}  // extern "C"
