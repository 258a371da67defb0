// qoc_run_blk.hip — the block chains and block gradient (qoc_blk.hpp): detection of the generators' invariant
// blocks, the live / dead block bookkeeping, and the launches of one propagate / grape_sensitivity / concurrent eval on
// them.  It routes to the block propagators (qoc_run_blku.hip) and the stored propagators (qoc_run_blkp.hip).
#include <numeric>

#include "qoc_blk_host.hpp"

namespace qoc_host {

// Connected components of the union sparsity pattern of A_0..A_nu (host copy, c->h_gen): rows i and k share a block
// whenever some A_j[i, k] or A_j[k, i] is nonzero.  Blocks of at most BLK_NBMAX rows turn the block path on
// (QOC_BLOCKS=0 keeps the dense chains); d_brow lists each block's rows in increasing order, blocks ordered by
// their first row, padded with -1 to NB = 2, 3 or 4.
int blk_detect(qoc_ctx* c) {
  c->blk_nb = 0;
  c->nblk = 0;
  c->blk_jr = 0;
  c->blk_real = false;
  c->nwb = 0;
  c->h_brow.clear();
  c->seg_pen_valid = false;  // the penalty's row masks follow the block layout (blkseg_pen)
  if (env_is("QOC_BLOCKS", "0")) return QOC_OK;
  const bool valu = env_is("QOC_BLOCKS", "valu");  // blocks of <= 4 rows on the VALU lanes (k_blk_*)
  // blocks of <= 2 rows on their real embedding (JR = 0, QOC_BLOCKS=real): one MFMA per term and no DPP swap, but
  // 4 columns per wave and 5 waves per cavity seed instead of 3; measured the same as the complex slots (cavity
  // chain 0.79 vs 0.78 ms), so the complex slots stay the default
  const bool real_req = env_is("QOC_BLOCKS", "real");
  const int N = c->N;
  const size_t NN = (size_t)N * N;
  std::vector<int> par(N);
  std::iota(par.begin(), par.end(), 0);
  auto find = [&](int x) {
    while (par[x] != x) x = par[x] = par[par[x]];
    return x;
  };
  for (int j = 0; j <= c->nu; ++j)
    for (int col = 0; col < N; ++col)
      for (int row = 0; row < N; ++row) {
        const double* v = c->h_gen.data() + 2 * (j * NN + row + (size_t)N * col);
        if (row != col && (v[0] != 0.0 || v[1] != 0.0)) {
          const int a = find(row), b = find(col);
          if (a != b) par[std::max(a, b)] = std::min(a, b);
        }
      }
  std::vector<std::vector<int>> blocks;
  std::vector<int> id(N, -1);
  for (int row = 0; row < N; ++row) {
    const int root = find(row);
    if (id[root] < 0) {
      id[root] = (int)blocks.size();
      blocks.emplace_back();
    }
    blocks[id[root]].push_back(row);
  }
  size_t mx = 0;
  for (const auto& bl : blocks) mx = std::max(mx, bl.size());
  // blocks of <= 4 rows: packed into the aligned 4-row slots of MFMA block waves (JR = 1), or one VALU lane per
  // (block, column) with QOC_BLOCKS=valu; 5..16 rows: one MFMA wave per block (JR = 4), only when the dense state
  // needs more than one 16-row group (N > 16: at N <= 16 the dense register chain already runs one wave per column
  // pair)
  if (mx > 16 || (mx > (size_t)BLK_NBMAX && N <= 16)) return QOC_OK;
  const int NB = mx <= 2 ? 2 : mx <= 3 ? 3 : mx <= 4 ? 4 : 16;
  const int nblk = (int)blocks.size();
  std::vector<int> brow((size_t)nblk * NB, -1);
  for (int b = 0; b < nblk; ++b)
    for (size_t i = 0; i < blocks[b].size(); ++i) brow[(size_t)b * NB + i] = blocks[b][i];
  // the MFMA waves' 16-row states
  std::vector<int> wrow;
  int jr = 0;
  bool real = false;
  if (NB == 16) {
    jr = 4;
    wrow = brow;
  } else if (real_req && mx <= 2) {
    // real embedding: a block of <= 2 complex rows is one 4-row slot [Re r0, Re r1, Im r0, Im r1] (two 1-row blocks
    // share a slot); entries row * 2 + part, so that each element's partner part sits 32 lanes away
    real = true;
    std::vector<int> rows;  // complex rows in slot order, 2 per slot (-1 padding)
    for (const auto& bl : blocks) {
      if (bl.size() == 2 && rows.size() % 2) rows.push_back(-1);  // a 2-row block starts a slot
      for (int r : bl) rows.push_back(r);
    }
    if (rows.size() % 2) rows.push_back(-1);
    for (size_t q = 0; q < rows.size(); q += 2) {
      const int r0 = rows[q], r1 = rows[q + 1];
      wrow.push_back(r0 >= 0 ? 2 * r0 : -1);
      wrow.push_back(r1 >= 0 ? 2 * r1 : -1);
      wrow.push_back(r0 >= 0 ? 2 * r0 + 1 : -1);
      wrow.push_back(r1 >= 0 ? 2 * r1 + 1 : -1);
    }
    while (wrow.size() % 16) wrow.push_back(-1);
  } else if (!valu) {
    jr = 1;
    std::vector<int> slot;  // rows of the 4-row slots, in order (a block never straddles two slots)
    int fill = 0;
    for (const auto& bl : blocks) {
      if (fill + (int)bl.size() > 4) {
        for (; fill < 4; ++fill) slot.push_back(-1);
        fill = 0;
      }
      for (int r : bl) slot.push_back(r);
      fill += (int)bl.size();
      if (fill == 4) fill = 0;
    }
    while (slot.size() % 16) slot.push_back(-1);
    wrow = slot;
  }
  c->h_wrow = wrow;
  c->h_brow = brow;
  c->h_wrow_live.clear();
  c->h_dead_rows.clear();
  c->dead_dirty = true;
  // the row lists and the table of a previous qoc_set_generators go first
  for (DevBufBase* b : {(DevBufBase*)&c->d_brow, (DevBufBase*)&c->d_wrow, (DevBufBase*)&c->d_wrow_live,
                        (DevBufBase*)&c->d_dead_rows, (DevBufBase*)&c->d_gtab})
    b->release();
  HIPCHK(c, c->d_brow.alloc(brow.size() * sizeof(int)));
  HIPCHK(c, hipMemcpy(c->d_brow, brow.data(), brow.size() * sizeof(int), hipMemcpyHostToDevice));
  if (NB <= 3) {
    // the segmented eval's generator blocks, block-major [nblk][3][NB^2]: the entries of the shifted generators
    // Ã_j = A_j - μ_j I (the values qoc_set_generators uploads to d_At: the same subtraction) on each block's rows,
    // zero for j > nu and for a padded row; its prologue copies the table instead of gathering through d_brow
    std::vector<double> tab((size_t)nblk * 3 * NB * NB * 2, 0.0);
    blk_gen_table(c, brow, NB, nblk, c->h_gen.data(), c->tprm.mur, c->tprm.mui, tab.data());
    HIPCHK(c, c->d_gtab.alloc(tab.size() * sizeof(double)));
    HIPCHK(c, hipMemcpy(c->d_gtab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  if (jr || real) {
    HIPCHK(c, c->d_wrow.alloc(wrow.size() * sizeof(int)));
    HIPCHK(c, hipMemcpy(c->d_wrow, wrow.data(), wrow.size() * sizeof(int), hipMemcpyHostToDevice));
  }
  c->blk_nb = NB;
  c->nblk = nblk;
  c->blk_jr = jr;
  c->blk_real = real;
  c->nwb = (int)(wrow.size() / 16);
  return QOC_OK;
}

void blk_gen_table(const qoc_ctx* c, const std::vector<int>& brow, int NB, int nblk, const double* gen,
                   const double* mur, const double* mui, double* tab) {
  const int N = c->N, E = NB * NB;
  const size_t NN = (size_t)N * N;
  std::fill(tab, tab + (size_t)nblk * 3 * E * 2, 0.0);
  for (int b = 0; b < nblk; ++b)
    for (int j = 0; j <= c->nu && j < 3; ++j)
      for (int e = 0; e < E; ++e) {
        const int ri = brow[(size_t)b * NB + e / NB], rk = brow[(size_t)b * NB + e % NB];
        if (ri < 0 || rk < 0) continue;
        const double* v = gen + 2 * (j * NN + ri + (size_t)N * rk);
        double* t = tab + 2 * (((size_t)b * 3 + j) * E + e);
        t[0] = ri == rk ? v[0] - mur[j] : v[0];
        t[1] = ri == rk ? v[1] - mui[j] : v[1];
      }
}

// The block path runs the Taylor-action chains' fp64 scheme (step records, shifted generators) on unpacked states
bool blk_active(const qoc_ctx* c) {
  if (c->blk_nb <= 0 || c->prec != QOC_FP64 || c->chain_mode != 1 || c->prop_method != QOC_PROP_EXPM || c->big ||
      c->packed || c->nu > 2)
    return false;
  // MFMA block waves: <= 8 per workgroup (the 512-thread launch bound keeps 256 VGPRs per wave)
  if (c->blk_real) return c->nwb * ((c->m + 3) / 4) <= 8;
  if (c->blk_jr) return c->nwb * ((c->m + 1) / 2) <= 8 && (c->blk_nb < 16 || tchain_mf(c));
  return c->nblk * c->m <= BLK_MAXT && c->nblk <= 256;
}
// MFMA block waves (k_blkrot_*): the chain kernels; blocks of 16 rows also take the dense gradient kernels
bool blk_rot(const qoc_ctx* c) { return c->blk_jr > 0 || c->blk_real; }

// Block propagators (qoc_blku.hpp, qoc_run_blku.hip), the default for blocks of <= 4 rows: formed per (slice, block)
// apart from the serial chain, which then runs one NB x NB matvec per slice.  QOC_BLKU=0 keeps the
// polynomial-in-the-chain kernels (k_blkrot_* / k_blk_*).  The gradient packs 64 / nblk slices per wave (nblk <= 32);
// the chain lanes take nblk m <= 256 (block, column) pairs.
bool blku_on(const qoc_ctx* c) {
  // QOC_BLOCKS=valu / real ask for those kernel variants explicitly (blk_jr != 1): they keep them
  if (!blk_active(c) || c->blk_jr != 1 || c->blk_nb > BLK_NBMAX || c->nu < 1 || c->nu > 2 || c->nblk > 32 ||
      c->nblk * c->m * (c->blk_nb == 2 ? 2 : 4) > 64 * (c->blk_nb == 4 ? 2 : 4))
    return false;
  // an explicit QOC_BLOCKS=valu / real keeps the polynomial-in-the-chain kernels, also where it falls back to the
  // complex MFMA slots (real with blocks of more than 2 rows)
  if (env_is("QOC_BLOCKS", "valu", "real")) return false;
  return !env_is("QOC_BLKU", "0");
}

// Stored / interpolating propagators for blocks of 5..16 rows (qoc_blkp.hpp, qoc_run_blkp.hip); QOC_BLKP=0 keeps the
// Chebyshev-action chains (k_blkrot_dual)
bool blkp_on(const qoc_ctx* c) {
  return blk_active(c) && blk_big(c) && c->nu >= 1 && c->nu <= 2 && env_int("QOC_BLKP", 1) != 0;
}

static int blk_threads(const qoc_ctx* c, int nwb = -1) {
  if (nwb < 0) nwb = c->nwb;
  if (c->blk_real) return 64 * nwb * ((c->m + 3) / 4);  // 4 state columns per real-embedded wave
  return blk_rot(c) ? 64 * nwb * ((c->m + 1) / 2) : 64 * ((c->nblk * c->m + 63) / 64);
}
static size_t blk_lds_of(const qoc_ctx* c, int nwb = -1) {
  return blk_rot(c) ? blkrot_lds(c->N, c->m, blk_threads(c, nwb) / 64) : blk_lds(c->N, c->m);
}

// Blocks of 5..16 rows that carry no state: x_0 (every seed) and X_target are zero on all their rows.  The generators
// keep every block invariant, so such a block's x_k and μ_k are exactly zero at every k, and it adds nothing to J
// (its overlaps are zero) or to dJ/du (each generator's contribution is λ_β^H A_jβ x_β = 0).  The reference exploits
// the same structure by hand with compress_states (src/utils.jl:96-109; the tunable bus' parity blocks,
// test/test_utils.jl:23): here the concurrent eval launches waves for the live blocks only and k_zero_rows writes
// the dead rows' zeros into the state-shaped buffers, so every output (x_k, λ_k, J, dJ/du) is what the full launch
// gives.  The tunable bus (m = 1, |110> -> |200>) carries its state in the 14-row even-parity block only.
// QOC_BLK_DEAD=0 launches every block.  Sets bk.wrow / bk.nwb; leaves them when every block is live.
// blk_live_rows: the host half: the live wave blocks' rows (16 per block) and the dead blocks' rows; false: every block
// counts as live
bool blk_live_rows(const qoc_ctx* c, std::vector<int>& wl, std::vector<int>& dead) {
  wl.clear();
  dead.clear();
  if (!blk_big(c) || c->h_wrow.empty() || c->h_Xt.empty() || !c->have_x0) return false;
  if (env_int("QOC_BLK_DEAD", 1) == 0) return false;
  const int N = c->N, mu = c->m_user;
  const size_t cnt = c->x0_per_seed ? (size_t)c->B : 1, Nmu = (size_t)N * mu;
  if (c->h_x0.size() < 2 * Nmu * cnt || c->h_Xt.size() < 2 * Nmu) return false;
  std::vector<char> live(N, 0);
  auto mark = [&](const double* v) {
    for (size_t e = 0; e < Nmu; ++e)
      if (v[2 * e] != 0.0 || v[2 * e + 1] != 0.0) live[e % N] = 1;
  };
  for (size_t q = 0; q < cnt; ++q) mark(c->h_x0.data() + 2 * Nmu * q);
  mark(c->h_Xt.data());
  for (int w = 0; w < c->nwb; ++w) {
    bool lv = false;
    for (int i = 0; i < 16; ++i) {
      const int r = c->h_wrow[16 * w + i];
      lv = lv || (r >= 0 && live[r]);
    }
    for (int i = 0; i < 16; ++i) {
      const int r = c->h_wrow[16 * w + i];
      if (lv) wl.push_back(r);
      else if (r >= 0) dead.push_back(r);
    }
  }
  return !(dead.empty() || wl.empty());
}
// all: every block counts as live (a co-state source puts λ_k on every row)
int blk_live(qoc_ctx* c, BlkArgs& bk, bool all) {
  std::vector<int> wl, dead;
  if (all || !blk_live_rows(c, wl, dead)) return QOC_OK;
  if (wl != c->h_wrow_live || dead != c->h_dead_rows) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->d_dead_rows.release();
    HIPCHK(c, c->d_wrow_live.alloc(wl.size() * sizeof(int)));
    HIPCHK(c, hipMemcpy(c->d_wrow_live, wl.data(), wl.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(c, c->d_dead_rows.alloc(dead.size() * sizeof(int)));
    HIPCHK(c, hipMemcpy(c->d_dead_rows, dead.data(), dead.size() * sizeof(int), hipMemcpyHostToDevice));
    c->h_wrow_live = wl;
    c->h_dead_rows = dead;
  }
  bk.wrow = c->d_wrow_live;
  bk.nwb = (int)(wl.size() / 16);
  return QOC_OK;
}
// the dead rows' zeros (blk_live) in up to six state-shaped buffers of B (Nt + 1) m columns.  A buffer that already
// holds zeros on the same rows is skipped: every exact recurrence keeps rows whose x0 and target are zero at zero
// (the generators keep the blocks invariant), so only a backward with an external λ_N or a co-state source
// (dead_dirty), new generators or a reallocated buffer can put anything else there.  Each caller names the buffers it
// is about to write and no others: a propagate leaves d_L, the co-states of the last grape_sensitivity (which
// qoc_get_costates still answers for, and which may live on rows that are dead by now), as it is.
bool blk_dead_pending(const qoc_ctx* c, const void* buf) {
  if (c->dead_dirty || c->h_dead_zeroed != c->h_dead_rows) return true;
  return std::find(std::begin(c->dead_bufs), std::end(c->dead_bufs), buf) == std::end(c->dead_bufs);
}
int blk_zero_dead(qoc_ctx* c, std::initializer_list<void*> bufs) {
  ZeroRows z{};
  for (void* p : bufs)
    if (p && z.nbuf < 6 && blk_dead_pending(c, p)) z.buf[z.nbuf++] = (double2*)p;
  if (c->dead_dirty || c->h_dead_zeroed != c->h_dead_rows)  // what the other buffers hold there is unknown now
    for (const void*& p : c->dead_bufs) p = nullptr;
  c->h_dead_zeroed = c->h_dead_rows;
  c->dead_dirty = false;
  if (!z.nbuf) return QOC_OK;
  const long long cols = (long long)c->B * (c->Nt + 1) * c->m;
  const long long total = cols * (long long)c->h_dead_rows.size();
  const unsigned grid = (unsigned)std::min<long long>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(k_zero_rows, dim3(grid), dim3(256), 0, c->stream, z, cols, c->N, c->d_dead_rows,
                     (int)c->h_dead_rows.size());
  HIPCHK(c, hipGetLastError());
  for (int i = 0; i < z.nbuf; ++i) {  // into a free slot (six buffers at the most are ever named: d_X, d_L, four captures)
    const void** slot = std::find(std::begin(c->dead_bufs), std::end(c->dead_bufs), (const void*)nullptr);
    if (slot == std::end(c->dead_bufs)) slot = c->dead_bufs + i;
    *slot = z.buf[i];
  }
  return QOC_OK;
}

// the kernel pair of one chain pass as blk_launch's selector: ROT<JR, CH> on MFMA block waves, VALU<NB, CH> on the lanes
#define BLK_KERNELS(ROT, VALU)                     \
  [](auto K_, auto CH_) {                          \
    constexpr int K = decltype(K_)::value;         \
    constexpr bool CH = decltype(CH_)::value;      \
    if constexpr (K < 100) return ROT<K, CH>;      \
    else return VALU<K - 100, CH>;                 \
  }
// One chain launch of `blocks` workgroups of `thr` threads on the engine stream.  sel(selector, Chebyshev) names the
// kernel: selector 0 / 1 / 4 = k_blkrot_*<JR> (dynamic LDS above the default), 102 / 103 / 104 = k_blk_*<NB>
template <typename S, typename... A>
static hipError_t blk_launch(const qoc_ctx* c, S sel, int blocks, int thr, size_t lds, const A&... a) {
  using std::integral_constant;
  auto go = [&](auto K_) {
    auto kern = c->fwd.steps_cheb ? sel(K_, std::true_type()) : sel(K_, std::false_type());
    const hipError_t q = decltype(K_)::value < 100 ? blk_lds_attr(kern, lds) : hipSuccess;
    if (q != hipSuccess) return q;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(thr), lds, c->stream, a...);
    return hipGetLastError();
  };
  if (c->blk_real) return go(integral_constant<int, 0>());
  if (c->blk_jr == 1) return go(integral_constant<int, 1>());
  if (c->blk_jr == 4) return go(integral_constant<int, 4>());
  switch (c->blk_nb) {
    case 2: return go(integral_constant<int, 102>());
    case 3: return go(integral_constant<int, 103>());
    case 4: return go(integral_constant<int, 104>());
  }
  return hipErrorInvalidValue;
}

int blk_forward(qoc_ctx* c) {
  if (blku_on(c)) return blku_forward(c);
  int r = blkp_forward(c);  // blocks of 5..16 rows: stored propagators (1: not applicable)
  if (r != 1) return r;
  r = tchain_prep(c);
  if (r) return r;
  const TChainArgs g = tchain_args(c);
  const BlkArgs bk = blk_args(c);
  const int mk = mark_begin(c, 1);
  const hipError_t e = blk_launch(c, BLK_KERNELS(k_blkrot_fwd, k_blk_fwd), c->B, blk_threads(c), blk_lds_of(c), g, bk);
  mark_end(c, mk);
  if (e != hipSuccess) return fail(c, QOC_ERR_HIP, "k_blk_fwd launch: %s", hipGetErrorString(e));
  c->props_since_reset++;
  return QOC_OK;
}

// the order-o gradient from d_X and d_L (mu_mode: d_L holds μ, λ = coef ⊙ μ with the coefficients in d_coef)
static int blk_grad(qoc_ctx* c, int order, bool mu_mode, double* d_dJdu) {
  const TChainArgs g = tchain_args(c);
  const BlkArgs bk = blk_args(c);
  const long long units = (long long)c->B * c->Nt;
  const int upw = 256 / c->nblk;
  if (upw < 1) return fail(c, QOC_ERR_UNSUPPORTED, "block gradient: %d blocks exceed one workgroup", c->nblk);
  const unsigned blocks = (unsigned)((units + upw - 1) / upw);
  const int mk = mark_begin(c, 3);
  auto launch = [&](auto NB_) {
    return blk_order_dispatch(order, [&](auto ORD_) {
      hipLaunchKernelGGL((k_blk_grad<decltype(NB_)::value, decltype(ORD_)::value>), dim3(blocks), dim3(256), 0,
                         c->stream, g, bk, units, (int)mu_mode, d_dJdu);
      return hipGetLastError();
    });
  };
  const hipError_t e = c->blk_nb == 2   ? launch(std::integral_constant<int, 2>())
                       : c->blk_nb == 3 ? launch(std::integral_constant<int, 3>())
                                        : launch(std::integral_constant<int, 4>());
  mark_end(c, mk);
  if (e != hipSuccess) return fail(c, QOC_ERR_HIP, "k_blk_grad launch: %s", hipGetErrorString(e));
  return QOC_OK;
}

// grape_sensitivity: λ by the block backward chain (penalty, co-state source and an external λ_N included), then the
// block gradient for orders 1..4; the exact (Fréchet) gradient runs its own dense kernel on the same λ.
int blk_backward(qoc_ctx* c, int order, double* d_dJdu) {
  if (blku_on(c)) return blku_backward(c, order, d_dJdu);
  if (c->fwd.steps_old) {  // the last forward was the stored-propagator eval (blkp): this u's step records first
    if (int r0 = tchain_prep(c)) return r0;
  }
  const TChainArgs g = tchain_args(c);
  const BlkArgs bk = blk_args(c);
  const int mk = mark_begin(c, 2);
  const hipError_t e = blk_launch(c, BLK_KERNELS(k_blkrot_bwd, k_blk_bwd), c->B, blk_threads(c), blk_lds_of(c), g, bk);
  mark_end(c, mk);
  if (e != hipSuccess) return fail(c, QOC_ERR_HIP, "k_blk_bwd launch: %s", hipGetErrorString(e));
  if (order == QOC_DUKDP_EXACT || blk_big(c)) return dense_gradient<double>(c, order, d_dJdu);
  return blk_grad(c, order, false, d_dJdu);
}

// qoc_eval_dev with a built-in cost, no penalty and no co-state source: the forward chain and the μ recurrence
// (λ_k = coef ⊙ μ_k, src/penalty_fcns.jl:19-22, 35-40) in one launch, then the gradient with the coefficients.  (With a
// penalty or a source λ_k needs x_k: the two directions run in sequence, qoc_propagate_dev then the backward.)
bool blk_concurrent_ok(const qoc_ctx* c, int order) {
  // MFMA block waves: the contraction from the chains' captures (k_grad_rr_c, order 3); the exact gradient on the
  // interpolating propagators of blocks of 5..16 rows (blkp_exact_on: blk_eval_concurrent may still return 1)
  const bool exact = order == QOC_DUKDP_EXACT && blk_big(c) && blkp_exact_on(c);
  if (blk_big(c) && !(order == 3 && tchain_cap_ok(c)) && !exact) return false;
  // (blocks of 5..16 rows: a penalty without a penalised entry in a live block is no penalty, blkp_pen_mode)
  return blk_active(c) && c->concurrent && ((order >= 1 && order <= BLK_ORDMAX) || exact) &&
         (c->cost_kind == QOC_COST_TRACE || c->cost_kind == QOC_COST_ZCAL) &&
         ((c->mu == 0.0 && !c->src_on) || (blkp_on(c) && blkp_pen_mode(c) == 0));
}

// The router of the concurrent eval: the block propagators (blocks of <= 4 rows), the stored propagators (5..16 rows),
// else the Chebyshev block chains, whose eval this is.  Returns 1, with nothing launched, for an exact eval whose
// interpolation does not apply (a control range the series cannot resolve): the caller runs propagate + backward
int blk_eval_concurrent(qoc_ctx* c, int order, double* d_dJdu) {
  if (blku_on(c)) return blku_eval_concurrent(c, order, d_dJdu);
  int r;
  if ((r = blk_coef_mu(c))) return r;
  if (blkp_on(c)) {
    BlkArgs bk = blk_args(c);
    if ((r = blk_live(c, bk))) return r;
    if (blkp_fits_nwb(c, bk.nwb)) {
      r = blkp_eval_concurrent(c, order, d_dJdu, bk);
      if (r != 1) return r;  // 1: the propagators do not fit in HBM: the Chebyshev block chains below
    }
  }
  if (order == QOC_DUKDP_EXACT) return 1;
  if ((r = blk_big(c) ? ensure_pws(c) : QOC_OK)) return r;
  if ((r = tchain_prep(c))) return r;
  TChainArgs gf = tchain_args(c);
  TChainArgs gb = tchain_args(c);
  gb.mu_mode = 1;
  if (blk_big(c)) {  // the first two products of every slice for k_grad_rr_c (forward -> d_pws, μ -> d_gws)
    const size_t bufN = (size_t)c->N * ((size_t)c->B * (c->Nt + 1) * c->m);
    gf.cap1 = c->d_pws;
    gf.cap2 = c->d_pws.as<cx<double>>() + bufN;
    gb.cap1 = c->d_gws;
    gb.cap2 = c->d_gws.as<cx<double>>() + bufN;
  }
  BlkArgs bk = blk_args(c);
  if ((r = blk_live(c, bk))) return r;
  if (bk.nwb != c->nwb) {
    if ((r = blk_zero_dead(c, {c->d_X, c->d_L, (void*)gf.cap1, (void*)gf.cap2, (void*)gb.cap1, (void*)gb.cap2})))
      return r;
  }
  const int mk = mark_begin(c, 1);
  const hipError_t e = blk_launch(c, BLK_KERNELS(k_blkrot_dual, k_blk_dual), 2 * c->B, blk_threads(c, bk.nwb),
                                  blk_lds_of(c, bk.nwb), gf, gb, bk);
  mark_end(c, mk);
  if (e != hipSuccess) return fail(c, QOC_ERR_HIP, "k_blk_dual launch: %s", hipGetErrorString(e));
  c->props_since_reset++;  // (no captures left for a later backward: the block backward recomputes its own products)
  if (blk_big(c)) {
    const int mg = mark_begin(c, 3);
    r = grad_rr_cap(c, d_dJdu, c->stream, 0, c->Nt, true);
    mark_end(c, mg);
  } else {
    r = blk_grad(c, order, true, d_dJdu);
  }
  if (r) return r;
  HIPCHK(c, hipMemcpyAsync(c->d_coef_mu, c->d_coef, (size_t)c->B * 2 * c->m * sizeof(cx<double>),
                           hipMemcpyDeviceToDevice, c->stream));
  c->bwd.is_mu = true;
  c->bwd.route = 4;
  return QOC_OK;
}

int blk_materialize(qoc_ctx* c) {
  int r = QOC_OK;
  if (c->fwd.lazy) r = blku_states(c);
  if (r == QOC_OK && c->bwd.lazy) r = blku_costates(c);
  return r;
}

}  // namespace qoc_host
