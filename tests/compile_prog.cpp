// compile_prog.cpp -- stand-alone driver of the model compiler (pednstream_amd/csrc/pedn_compile.hpp) for tests/test_model_compile_host.py:
// built with the host compiler and ASan + UBSan, no HIP library linked, nothing stepped.
//
//   compile_prog <model file> <n_replicas> [lds_limit=N] [heavy_groups=N] [pack_by_load=N] [general_degree=1]
//
// The model file (tests/compile_model.py writes it from the dict of flatten_network) has one array per line: name, type (i int32,
// d binary64 as hex bits, f binary32 as hex bits), count, values.  Arrays named dead0, dead1, ... are sets of nodes ([n_nodes] 0 / 1): for
// each, the live nodes are repacked from the full packing's records the way dl_refresh does it.  Prints "key: values" lines.
#include <stdio.h>

#include <fstream>
#include <map>
#include <sstream>

#include "../pednstream_amd/csrc/pedn_compile.hpp"

struct ModelFile {
  std::map<std::string, std::vector<int32_t>> i;
  std::map<std::string, std::vector<double>> d;
  std::map<std::string, std::vector<float>> f;
  pedn_model_desc desc{};

  bool read(const char* path) {
    std::ifstream in(path);
    if (!in) return false;
    std::string line;
    while (std::getline(in, line)) {
      std::istringstream ss(line);
      std::string name, type;
      size_t n = 0;
      if (!(ss >> name >> type >> n)) continue;
      if (type == "i") {
        std::vector<int32_t>& a = i[name];
        a.resize(n);
        for (size_t k = 0; k < n; ++k) ss >> a[k];
      } else if (type == "d") {
        std::vector<double>& a = d[name];
        a.resize(n);
        for (size_t k = 0; k < n; ++k) { uint64_t b = 0; ss >> std::hex >> b; memcpy(&a[k], &b, 8); }
      } else {
        std::vector<float>& a = f[name];
        a.resize(n);
        for (size_t k = 0; k < n; ++k) { uint32_t b = 0; ss >> std::hex >> b; memcpy(&a[k], &b, 4); }
      }
      if (!ss) return false;
    }
    // arrays are handed out at their exact size, so that a read past a table's end is a heap overflow the sanitizer sees
    pedn_model_desc& m = desc;
#define S(x) m.x = i.at(#x).at(0)
#define SD(x) m.x = d.at(#x).at(0)
#define I(x) m.x = i.at(#x).data()
#define D(x) m.x = d.at(#x).data()
    S(abi_version); S(n_nodes); S(n_links); S(n_vlinks); S(n_turns); S(n_demand); S(n_od); S(T); S(window); SD(dt);
    I(node_kind); I(node_slot_ptr); I(node_turn_ptr); I(node_demand_row); I(node_dyn); I(slot_in_link); I(slot_out_link);
    I(link_rev); I(link_sep); I(link_fd); I(link_tau_sw); I(link_fft);
    m.link_tt0 = f.at("link_tt0").data();
    D(link_length); D(link_width); D(link_vf); D(link_kc); D(link_kj); D(link_gamma); D(link_act); D(link_bi); D(link_noise);
    D(front_gate0); D(back_gate0); D(sep_width0); D(tf_init); D(demand); D(od_w);
    SD(pf_temp); SD(pf_alpha); SD(pf_beta); SD(pf_omega); SD(pf_eps);
    S(n_up); S(n_upod); S(n_grp); S(n_ent); S(n_pair);
    I(node_up_ptr); I(up_slot); I(up_od_ptr); I(upod_od); I(node_grp_ptr); I(grp_ent_ptr); I(grp_allphys); I(grp_node); I(ent_link);
    D(ent_dist); I(turn_pair_ptr); I(pair_ent); I(pair_upod);
    S(history_mode); S(node_model);
    m.node_cost = f.count("node_cost") ? f.at("node_cost").data() : nullptr;
#undef S
#undef SD
#undef I
#undef D
    return true;
  }
};

template <typename T>
static void put(const char* key, const T* a, size_t n) {
  printf("%s:", key);
  for (size_t k = 0; k < n; ++k) printf(" %lld", (long long)a[k]);
  printf("\n");
}
template <typename T>
static void put(const char* key, const std::vector<T>& a) { put(key, a.data(), a.size()); }

template <typename T>
static void put_words(const char* key, const std::vector<T>& a) {   // records without padding, as 32-bit words
  static_assert(sizeof(T) % 4 == 0, "whole words");
  printf("%s:", key);
  for (const T& x : a) {
    uint32_t w[sizeof(T) / 4];
    memcpy(w, &x, sizeof(T));
    for (uint32_t u : w) printf(" %x", u);
  }
  printf("\n");
}

static void put_packing(const std::string& prefix, const pedn_compile::Packing& P) {
  const int info[5] = {P.n_blocks, P.tiles, P.n_lp, P.lp_max_m, (int)P.rec.size()};
  put((prefix + "info").c_str(), info, 5);
  for (size_t k = 0; k < P.rec.size(); ++k) {   // field by field, then the two links' parameters as words
    const SlotRec& R = P.rec[k];
    const int32_t f[14] = {R.node, R.slot, R.base, R.m, R.kind, R.dyn, R.lin, R.lout, R.turn0, R.demand_row, R.act, R.lp, R.trow, R.mirror};
    put((prefix + "rec").c_str(), f, 14);
    put_words((prefix + "recP").c_str(), std::vector<LinkP>{R.Pin, R.Pout});
  }
}

static void put_tables(const pedn_compile::Tables& t) {
  const int info[8] = {t.n_multi, t.n_trow, t.n_over, t.n_tf_heavy_quads, t.inline_tf_ok, t.packed_by, t.max_degree, t.pairs_adj};
  put("info", info, 8);
  put("m64", t.m64, 7); put("m32", t.m32, 6); put("rows64", t.rows64, 7); put("rows32", t.rows32, 6);
  put("pair_const", t.pair_const); put("turn_mode", t.turn_mode); put("slot_dyn", t.slot_dyn); put("slot_trow", t.slot_trow);
  put("trow_words", t.trow_words); put("tgrp_words", t.tgrp_words); put("pair_row", t.pair_row);
  put("demand_nz", t.demand_nz); put("pack_order", t.pack_order);
  put_words("lp", t.lp); put_words("corr", t.corr);
  put_packing("full_", t.full);
}

// ---- main
int main(int argc, char** argv) {
  if (argc < 3) return 2;
  ModelFile mf;
  if (!mf.read(argv[1])) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  const int n_replicas = atoi(argv[2]);
  pedn_compile::Options opt;
  for (int a = 3; a < argc; ++a) {
    const std::string arg = argv[a];
    const size_t eq = arg.find('=');
    if (eq == std::string::npos) return 2;
    const std::string key = arg.substr(0, eq);
    const int val = atoi(arg.c_str() + eq + 1);
    if (key == "lds_limit") opt.tf_lds_limit = val;
    else if (key == "heavy_groups") opt.tf_heavy_groups = val;
    else if (key == "pack_by_load") opt.pack_by_load = val;
    else if (key == "general_degree") opt.general_degree = val != 0;
    else return 2;
  }
  std::string err;
  pedn_compile::Tables t;
  int rc = pedn_compile::validate(mf.desc, n_replicas, &err);
  if (rc == PEDN_OK) rc = pedn_compile::compile(mf.desc, opt, &t, &err);
  printf("rc: %d\nerr: %s\n", rc, err.c_str());
  if (rc != PEDN_OK) return 0;
  put_tables(t);
  // the live packings: the full packing's records of the nodes outside each given set
  const std::vector<SlotRec>& full = t.full.rec;
  std::vector<int32_t> first(mf.desc.n_nodes, -1);
  for (size_t k = 0; k < full.size(); ++k)
    if (full[k].node >= 0 && full[k].slot == 0) first[full[k].node] = (int32_t)k;
  for (int k = 0;; ++k) {
    const std::string name = "dead" + std::to_string(k);
    if (!mf.i.count(name)) break;
    const std::vector<char> dead(mf.i[name].begin(), mf.i[name].end());
    put_packing("live" + std::to_string(k) + "_", pedn_compile::pack(t.pack_order, mf.desc.node_slot_ptr, dead.data(), mf.desc.n_links, true, false,
                                                                     [&](int n, int s) { return full[first[n] + s]; }));
  }
  return 0;
}
