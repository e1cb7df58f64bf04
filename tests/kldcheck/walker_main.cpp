// tests/kldcheck/walker_main.cpp -- TEST-ONLY stand-alone program: the planner of
// csrc/vbhmm_kld_plan.h and the host walk of its tiles (tests/checklib/kld_walk.h) on seeded
// inputs, for a run under the address and undefined-behaviour sanitizers on the CPU
// (`make kld_sanitize`; plain C++, no device compiler).  Lists of 0, 1, 127, 128, 129, 130
// and 257 items (reversed, repeated, strided), short jobs packed up to exactly 128 lanes
// and one item over, a list shared by many jobs, a == b, and every refusal: an index of
// -1, an index equal to its bound (HMM a, HMM b, list, item), decreasing offsets.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "host_prepare.h"
#include "kld_walk.h"
#include "walker_input.h"

using namespace vbhem::score;
using vbhem::kld::Plan;
using walker::Lcg;

namespace {

constexpr int H = 6, KM = 3, D = 2, N = 300;

struct Inputs {
  std::vector<int> nstates, offsets;
  std::vector<double> prior, trans, mean, cov, x;
  Layout L;
  std::vector<double> blocks;
};

Inputs make_inputs() {
  Inputs in;
  Lcg g{11};
  in.nstates = {3, 2, 3, 1, 3, 2};
  in.prior.assign(H * KM, 0.0);
  in.trans.assign(H * KM * KM, 0.0);
  in.mean.assign(H * KM * D, 0.0);
  in.cov.assign(H * KM * D, 1.0);
  for (int h = 0; h < H; ++h) {
    const int K = in.nstates[h];
    for (int k = 0; k < K; ++k) {
      in.prior[h * KM + k] = 1.0 / K;
      for (int j = 0; j < K; ++j) in.trans[(h * KM + k) * KM + j] = (j == k ? 0.5 : 0.0) + 0.5 / K;
      for (int a = 0; a < D; ++a) {
        in.mean[(h * KM + k) * D + a] = 4.0 * g.uni();
        in.cov[(h * KM + k) * D + a] = 0.5 + g.uni();
      }
    }
  }
  in.offsets.assign(N + 1, 0);
  for (int n = 0; n < N; ++n) in.offsets[n + 1] = in.offsets[n] + 1 + (int)(3 * g.uni());
  in.x.resize((size_t)in.offsets[N] * D);
  for (double &v : in.x) v = 4.0 * g.uni() + 0.8 * g.normal();
  in.L = make_layout(KM, D);
  if (checklib::host_prepare(in.L, H, KM, D, VBHEM_COV_DIAG, in.nstates.data(), in.prior.data(), in.trans.data(),
                             in.mean.data(), in.cov.data(), in.blocks))
    std::printf("host_prepare refused a covariance\n");
  return in;
}

template <int KB, int DB>
double straight(const Inputs &in, int a, int b, const int *items, int c) {
  const Hmm ma = view(in.L, in.blocks.data() + (size_t)a * in.L.stride, true);
  const Hmm mb = view(in.L, in.blocks.data() + (size_t)b * in.L.stride, true);
  double sum = 0.0;
  for (int q = 0; q < c; ++q) {
    const int off = in.offsets[items[q]], T = in.offsets[items[q] + 1] - off;
    const double own = pair_loglik<KB, DB>(ma, in.x.data() + (size_t)off * D, T, D) / (double)T;
    sum += vbhem::ccfd::kl_term(own, pair_loglik<KB, DB>(mb, in.x.data() + (size_t)off * D, T, D), T);
  }
  return sum / (double)c;
}

struct Case {
  std::vector<int> offsets{0}, items, jobs;
  int list(const std::vector<int> &it) {
    items.insert(items.end(), it.begin(), it.end());
    offsets.push_back((int)items.size());
    return (int)offsets.size() - 2;
  }
  void job(int a, int b, int l) {
    jobs.push_back(a);
    jobs.push_back(b);
    jobs.push_back(l);
  }
};

std::vector<int> gathered(int c, int kind) {
  std::vector<int> it((size_t)c);
  for (int q = 0; q < c; ++q)
    it[q] = kind == 0 ? (N - 1 - q) % N : kind == 1 ? (7 * q) % N : (q / 2 * 3) % N;  // reversed, strided, repeated
  return it;
}

int run_case(const Inputs &in, const Case &c, const char *name) {
  const int P = (int)c.jobs.size() / 3, nl = (int)c.offsets.size() - 1;
  Plan p;
  if (vbhem::kld::make_plan(H, N, nl, c.offsets.data(), c.items.data(), P, c.jobs.data(), p) != VBHEM_OK) {
    std::printf("%s: refused: %s\n", name, p.error.c_str());
    return 1;
  }
  Plan sized;
  int bad = vbhem::kld::make_plan(-1, -1, nl, c.offsets.data(), nullptr, P, c.jobs.data(), sized) != VBHEM_OK;
  bad += vbhem::kld::ws_layout(sized).total != vbhem::kld::ws_layout(p).total;
  const std::vector<char> tables = vbhem::kld::pack_tables(p, vbhem::kld::ws_layout(p));
  bad += tables.size() != vbhem::kld::ws_layout(p).total - vbhem::kld::ws_layout(p).tables;
  std::vector<int> first;
  const long long pairs = kldwalk::pair_firsts(P, c.jobs.data(), c.offsets.data(), first);
  std::vector<double> kl((size_t)P, -7.0);
  std::vector<int> own_hits((size_t)p.own_len, 0), pair_hits((size_t)pairs, 0);
  kldwalk::Walk{in.L, in.blocks, D, true, in.offsets.data(), in.x.data(), p, first.data(), kl.data(), own_hits.data(),
                pair_hits.data()}
      .operator()<4, 2>();
  for (int v : own_hits) bad += v != 1;
  for (int v : pair_hits) bad += v != 1;
  bad += pairs != p.n_lanes;
  for (int j = 0; j < P; ++j) {
    const int l = c.jobs[3 * j + 2], n = c.offsets[l + 1] - c.offsets[l];
    const double want = straight<4, 2>(in, c.jobs[3 * j], c.jobs[3 * j + 1], c.items.data() + c.offsets[l], n);
    bad += !(std::memcmp(&want, &kl[j], sizeof(double)) == 0 || (std::isnan(want) && std::isnan(kl[j])));
    bad += n > 0 && !std::isfinite(kl[j]);
  }
  std::printf("%s: jobs=%d own=%lld lanes=%lld tiles=%zu+%zu bad=%d\n", name, P, p.own_len, p.n_lanes,
              p.own_tiles.size(), p.cross_tiles.size(), bad);
  return bad;
}

int refused(const Case &c, int nl, const char *needle, const char *name) {
  Plan p;
  const int rc = vbhem::kld::make_plan(H, N, nl, c.offsets.data(), c.items.data(), (int)c.jobs.size() / 3,
                                       c.jobs.data(), p);
  const int bad = !(rc == VBHEM_ERR_ARG && p.error.find(needle) != std::string::npos && p.own_seq.empty());
  std::printf("%s: status=%d \"%s\" bad=%d\n", name, rc, p.error.c_str(), bad);
  return bad;
}

}  // namespace

int main() {
  const Inputs in = make_inputs();
  int bad = 0;
  {  // the edge lengths, every kind of gathering, a == b, an empty list between them
    Case c;
    const int lens[] = {1, 127, 128, 129, 130, 257};
    for (int i = 0; i < 6; ++i) {
      const int l = c.list(gathered(lens[i], i % 3));
      c.job(i % H, (i + 1) % H, l);
      c.job((i + 2) % H, (i + 1) % H, l);
      c.job(i % H, i % H, l);
      if (i == 2) c.job(1, 2, c.list({}));
    }
    bad += run_case(in, c, "edge lists");
  }
  {  // short jobs of one b packed to exactly 128 lanes, then one item over
    Case c;
    const int l60 = c.list(gathered(60, 1)), l8 = c.list(gathered(8, 0)), l9 = c.list(gathered(9, 2));
    c.job(0, 3, l60); c.job(1, 3, l60); c.job(2, 3, l8);   // 128
    c.job(0, 4, l60); c.job(1, 4, l60); c.job(2, 4, l9);   // 129
    bad += run_case(in, c, "packing");
  }
  {  // a list shared by many jobs, more jobs of one b than a tile has lanes, b not in order
    Case c;
    const int l = c.list(gathered(3, 0)), e = c.list({}), one = c.list({5});
    for (int j = 0; j < 300; ++j) c.job(j % H, (j * 5 + 1) % H, j % 7 == 0 ? e : j % 3 ? l : one);
    bad += run_case(in, c, "shared list");
  }
  {  // no jobs
    Case c;
    c.list({1, 2});
    bad += run_case(in, c, "no jobs");
  }
  {  // refusals
    Case c;
    const int l = c.list({0, 1, 2});
    auto with = [&](int a, int b, int li) {
      Case r = c;
      r.job(0, 1, l);
      r.job(a, b, li);
      return r;
    };
    bad += refused(with(-1, 0, l), 1, "job 1: HMM a = -1", "a = -1");
    bad += refused(with(H, 0, l), 1, "job 1: HMM a = 6", "a = H");
    bad += refused(with(0, -1, l), 1, "job 1: HMM b = -1", "b = -1");
    bad += refused(with(0, H, l), 1, "job 1: HMM b = 6", "b = H");
    bad += refused(with(0, 1, -1), 1, "job 1: list -1", "list = -1");
    bad += refused(with(0, 1, 1), 1, "job 1: list 1", "list = n_lists");
    Case neg = c, top = c, dec = c;
    neg.job(0, 1, neg.list({3, -1}));
    bad += refused(neg, 2, "list 1 item 1: sequence -1", "item = -1");
    top.job(0, 1, top.list({N}));
    bad += refused(top, 2, "list 1 item 0: sequence 300", "item = N");
    dec.offsets = {0, 3, 2};
    dec.job(0, 1, 0);
    bad += refused(dec, 2, "list offsets decrease at list 1", "decreasing offsets");
    Case unused = c;  // a list no job uses is not checked
    unused.list({-5, N + 7});
    unused.job(0, 1, l);
    bad += run_case(in, unused, "unused list");
  }
  std::printf(bad ? "FAILED %d\n" : "walker OK\n", bad);
  return bad != 0;
}
