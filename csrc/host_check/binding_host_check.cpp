// Host-only sanitizer harness for the launch-validation layer (csrc/binding.cpp).
//
// The binding is the only thing between Python and a hand-written kernel's grid: it must
// reject every call whose shapes the kernel does not support, and pass every pointer with
// the extent the kernel will touch.  Here it is compiled with g++ -fsanitize=address,undefined
// against CPU ATen (FD_HOST_VALIDATION), with the fd_* launchers replaced by stubs that
// (a) count calls and (b) check that every region the real kernel would read or write --
// derived from the launch arguments exactly as the kernel derives it -- lies inside a buffer
// the test registered.  The driver then makes valid calls (no exception, no violation) and
// invalid ones (a c10::Error, and NO launcher call).  Run by tests/test_host_sanitizers.py.
#define FD_HOST_VALIDATION 1
#include <algorithm>
#include "../binding.cpp"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

namespace hc {
struct Region { uintptr_t lo, hi; };
std::vector<Region> regions;
std::vector<std::string> violations;
int calls = 0;

void reg(const at::Tensor& t) {
  const uintptr_t p = reinterpret_cast<uintptr_t>(t.data_ptr());
  regions.push_back({p, p + (uintptr_t)(t.numel() * t.element_size())});
}
void span(const void* p, long long bytes, const char* what) {
  if (bytes <= 0) return;
  if (!p) { violations.push_back(std::string("null ") + what); return; }
  const uintptr_t lo = reinterpret_cast<uintptr_t>(p), hi = lo + (uintptr_t)bytes;
  for (const Region& r : regions)
    if (lo >= r.lo && hi <= r.hi) return;
  violations.push_back(std::string("out of bounds: ") + what + " (" + std::to_string(bytes) + " B)");
}
void opt_span(const void* p, long long bytes, const char* what) { if (p) span(p, bytes, what); }
// the hyper-parameters of an Adam step as the real launchers check them first (adam_epi.h
// fd_adam_hyper_rc): the stubs stand for the launchers, so a descriptor one of them would refuse is a
// violation -- the binding let it through
void hyper(const FdAdamHyper* h, const char* what) {
  if (!h) violations.push_back(std::string(what) + ": no hyper-parameters");
  else if (const int rc = fd_adam_hyper_rc(h))
    violations.push_back(std::string(what) + ": hyper-parameters out of range (rc=" + std::to_string(rc) + ")");
}
}  // namespace hc

// ------------------------------------------------------------------ stub launchers
extern "C" {
const void* g_hc_pf = nullptr;
long long g_hc_pf_bytes = 0;
int fd_gemm_pf(const void* pf, long long bytes) {
  g_hc_pf = pf;
  g_hc_pf_bytes = pf ? bytes : 0;
  return 0;
}
int fd_gemm_ex(int kind, int epi, const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb,
               int ldc, const float* bias, void* aux, int ldaux, const void* res, int ldres, float* workspace,
               long long workspace_elems, int accumulate, const FdAdamEpi* adam,
               float* colsum, int* colsum_blocks, void* aux_out, hipStream_t) {
  ++hc::calls;
  if (g_hc_pf) hc::span(g_hc_pf, g_hc_pf_bytes, "gemm prefetch");  // (the launch's one-shot prefetch)
  g_hc_pf = nullptr;
  g_hc_pf_bytes = 0;
  if (kind == 0) {  // A [M][lda] (K used), B [N][ldb], C [M][ldc] bf16
    hc::span(A, ((long long)(M - 1) * lda + K) * 2, "gemm A");
    hc::span(B, ((long long)(N - 1) * ldb + K) * 2, "gemm B");
  } else if (kind == 1) {  // A [M][lda], B [K][ldb] (N used)
    hc::span(A, ((long long)(M - 1) * lda + K) * 2, "gemm A");
    hc::span(B, ((long long)(K - 1) * ldb + N) * 2, "gemm B");
  } else {  // A [K][lda] (M used), B [K][ldb]
    hc::span(A, ((long long)(K - 1) * lda + M) * 2, "gemm A");
    hc::span(B, ((long long)(K - 1) * ldb + N) * 2, "gemm B");
  }
  hc::span(C, ((long long)(M - 1) * ldc + N) * (kind == 2 ? 4 : 2), "gemm C");
  if (epi == 1 || epi == 2) hc::span(bias, (long long)N * 4, "gemm bias");
  // (epi 2: u is optional -- the kernel writes it only when given)
  if (epi == 3 || (epi == 2 && aux)) hc::span(aux, ((long long)(M - 1) * ldaux + N) * 2, "gemm aux");
  if (epi == 4) hc::span(res, ((long long)(M - 1) * ldres + N) * 2, "gemm res");
  if (aux_out) hc::span(aux_out, ((long long)(M - 1) * ldaux + N) * 2, "gemm aux_out");
  if (colsum && colsum_blocks) {
    *colsum_blocks = (M + 127) / 128;
    hc::span(colsum, (long long)*colsum_blocks * N * 4, "gemm colsum");
  }
  if (kind == 2 && workspace_elems > 0) hc::span(workspace, workspace_elems * 4, "gemm workspace");
  if (adam && adam->p) {
    hc::span(adam->p, (long long)M * N * 4, "adam p");
    hc::span(adam->m, (long long)M * N * 4, "adam m");
    hc::span(adam->v, (long long)M * N * 4, "adam v");
    hc::opt_span(adam->sh, (long long)M * N * 2, "adam shadow");
  }
  (void)accumulate;
  return 0;
}
int fd_gemm(int kind, int epi, const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc,
            const float* bias, void* aux, int ldaux, const void* res, int ldres, float* workspace,
            long long workspace_elems, int accumulate, const FdAdamEpi* adam,
            float* colsum, int* colsum_blocks, hipStream_t st) {
  return fd_gemm_ex(kind, epi, A, B, C, M, N, K, lda, ldb, ldc, bias, aux, ldaux, res, ldres, workspace,
                    workspace_elems, accumulate, adam, colsum, colsum_blocks, nullptr, st);
}
int fd_gemm_set_cfg(int, int, int) { return 0; }
int fd_gemm_stamps(unsigned long long*, int) { return -1; }
int fd_attn_stamps(unsigned long long*, int) { return -1; }
int fd_attn_set_split(int) { return 0; }
int fd_gemm_dw2(const void* A0, const void* B0, float* C0, int M0, int N0, const void* A1, const void* B1, float* C1,
                int M1, int N1, int K, float* workspace, long long workspace_elems, int,
                const FdAdamEpi* adams, int, int* splits_out, hipStream_t) {
  ++hc::calls;
  hc::span(A0, (long long)K * M0 * 2, "dw2 A0");
  hc::span(B0, (long long)K * N0 * 2, "dw2 B0");
  hc::span(C0, (long long)M0 * N0 * 4, "dw2 C0");
  hc::span(A1, (long long)K * M1 * 2, "dw2 A1");
  hc::span(B1, (long long)K * N1 * 2, "dw2 B1");
  hc::span(C1, (long long)M1 * N1 * 4, "dw2 C1");
  hc::opt_span(workspace, workspace_elems * 4, "dw2 workspace");
  (void)adams;
  if (splits_out) *splits_out = 0;
  return 0;
}
int fd_gemm_dw2_splits(int, int, int, int, int) { return 1; }
int fd_gemm_dw_batch(int n, const FdDwProb* probs, int K, const int* step, const FdAdamHyper* h, int cfg,
                     const FdAdamRest* rest, hipStream_t) {
  ++hc::calls;
  if (h) hc::hyper(h, "dw_batch");  // (nullptr: no fused Adam -- and so neither a schedule nor a proximal term)
  const float prox_mu = h ? h->mu : 0.f;
  if (rest) {
    if (!h || !step) hc::violations.push_back("dw_batch rest without the fused Adam");
    if (rest->runs) hc::span(rest->runs, (long long)rest->nruns * 3 * 8, "dw_batch rest runs");
    if (rest->run_wd) hc::span(rest->run_wd, (long long)rest->nruns * 4, "dw_batch rest run decays");
    if (rest->wwd != 0.f && (!rest->ever || !h || !h->decoupled))
      hc::violations.push_back("dw_batch: a decaying sparse word table without flags / decoupled decay");
    if (rest->ever) {
      hc::span(rest->ever, rest->wrows, "dw_batch rest ever");
      hc::span(rest->now, rest->wrows, "dw_batch rest now");
      hc::span(rest->p + rest->woff, (long long)rest->wrows * rest->wrow4 * 16, "dw_batch rest word rows");
    }
    if (prox_mu != 0.f) {  // the anchor arena: the word rows and every run, at the offsets of p
      if (rest->ever && rest->wwd != 0.f) hc::violations.push_back("dw_batch: a proximal term on a decaying sparse word table");
      if (!rest->anchor) hc::violations.push_back("dw_batch: a proximal term without the rest's anchor");
      else if (rest->ever)
        hc::span(rest->anchor + rest->woff, (long long)rest->wrows * rest->wrow4 * 16, "dw_batch rest word anchor");
      for (int i = 0; rest->anchor && rest->runs && i < rest->nruns; ++i)
        hc::span(rest->anchor + 4 * rest->runs[3 * i], rest->runs[3 * i + 1] * 16, "dw_batch rest run anchor");
    }
  }
  if (n <= 0 || n > 32) hc::violations.push_back("dw_batch: problem count");
  for (int i = 0; i < n; ++i) {
    const FdDwProb& q = probs[i];
    const long long mn = (long long)q.M * q.N;
    const long long Kq = q.K > 0 ? q.K : K;
    if (Kq % 64) hc::violations.push_back("dw_batch: K % 64");
    hc::span(q.A, Kq * q.M * 2, "dw_batch A");
    hc::span(q.B, Kq * q.N * 2, "dw_batch B");
    hc::opt_span(q.bias, (long long)q.M * 4, "dw_batch bias");
    if (q.p) {
      hc::span(q.p, mn * 4, "dw_batch adam p");
      hc::span(q.m, mn * 4, "dw_batch adam m");
      hc::span(q.v, mn * 4, "dw_batch adam v");
      hc::opt_span(q.sh, mn * 2, "dw_batch adam shadow");
      if (prox_mu != 0.f) hc::span(q.anchor, mn * 4, "dw_batch adam anchor");
      if (prox_mu != 0.f && q.bias && rest && rest->anchor && rest->g)
        hc::span(rest->anchor + (q.bias - rest->g), (long long)q.M * 4, "dw_batch bias anchor");
      hc::span(step, 4, "dw_batch step");
      if (!h) hc::violations.push_back("dw_batch: fused Adam without hyper-parameters");
      if (!(q.wd >= 0.f) || !(q.bias_wd >= 0.f)) hc::violations.push_back("dw_batch: negative / NaN weight decay");
    } else {
      hc::span(q.C, mn * 4, "dw_batch C");
    }
  }
  (void)cfg;
  return 0;
}
int fd_adam_rows(float* p, const float* g, float* m, float* v, void* shadow, int rows, int row_len, const int* step,
                 const FdAdamHyper* h, const unsigned char* ever, const unsigned char* now, const float* anchor,
                 hipStream_t) {
  ++hc::calls;
  hc::hyper(h, "adam_rows");
  if (!h) return 0;
  const float wd = h->wd, prox_mu = h->mu;
  const int decoupled = h->decoupled;
  if (prox_mu != 0.f) hc::span(anchor, (long long)rows * row_len * 4, "adam_rows anchor");
  if (prox_mu != 0.f && wd != 0.f) hc::violations.push_back("adam_rows: a proximal term on a decaying table");
  if (wd != 0.f && !decoupled) hc::violations.push_back("adam_rows: coupled weight decay on flagged rows");
  const long long n = (long long)rows * row_len;
  hc::span(p, n * 4, "adam_rows p");
  hc::span(g, n * 4, "adam_rows g");
  hc::span(m, n * 4, "adam_rows m");
  hc::span(v, n * 4, "adam_rows v");
  hc::opt_span(shadow, n * 2, "adam_rows shadow");
  hc::span(step, 4, "adam_rows step");
  hc::span(ever, rows, "adam_rows ever");
  hc::opt_span(now, rows, "adam_rows now");
  return 0;
}
int fd_adam_lazy_decay(float* p, void* shadow, int* done, const unsigned char* ever, int rows, int row_len,
                       const int* step, int adj, const FdAdamHyper* h, const void* ids, int ids64, long long n,
                       hipStream_t) {
  ++hc::calls;
  hc::hyper(h, "lazy decay");
  const long long tot = (long long)rows * row_len;
  hc::span(p, tot * 4, "lazy decay p");
  hc::opt_span(shadow, tot * 2, "lazy decay shadow");
  hc::span(done, (long long)rows * 4, "lazy decay done");
  hc::span(ever, rows, "lazy decay ever");
  hc::span(step, 4, "lazy decay step");
  if (ids) hc::span(ids, n * (ids64 ? 8 : 4), "lazy decay ids");
  if (adj < 0 || adj > 1) hc::violations.push_back("lazy decay: adj");
  return 0;
}
int fd_gemm_splitk(int epi, const void* A, const void* Bt, int M, int N, int K, float* workspace,
                   long long workspace_elems, int splits, const float* bias, void* C, void* aux, void* aux_out,
                   const void* res, float* colsum, int* colsum_blocks, const FdLnEpi* ln, const FdSkHead* hd,
                   int b_mn, hipStream_t) {
  ++hc::calls;
  (void)b_mn;  // (W [K][N] or W^T [N][K]: the same N * K elements)
  const long long mn = (long long)M * N;
  if (hd && hd->W) {  // the fused head (FdSkHead): B rows of head outputs, M rows of partials
    hc::span(hd->W, (long long)2 * N * 4, "splitk head W");
    hc::span(hd->labels, (long long)hd->B * 8, "splitk head labels");
    hc::span(hd->logits, (long long)hd->B * 8, "splitk head logits");
    hc::span(hd->dlogits, (long long)hd->B * 8, "splitk head dlogits");
    hc::span(hd->dz, mn * 2, "splitk head dz");
    hc::opt_span(hd->dx, mn * 2, "splitk head dx");
    hc::span(hd->colpart, mn * 3 * 4, "splitk head colpart");
    hc::span(hd->hpart, mn * 2 * 4, "splitk head hpart");
    hc::span(hd->dbpart, (long long)M * 8, "splitk head dbpart");
    hc::span(hd->lpart, (long long)M * 4, "splitk head lpart");
    hc::span(hd->loss, 4, "splitk head loss");
    hc::span(hd->ticket, 4, "splitk head ticket");
    hc::opt_span(hd->own, (long long)(hd->B + 1) * 4, "splitk head own");
  }
  if (splits <= 0) splits = 1;
  hc::span(A, (long long)M * K * 2, "splitk A");
  hc::span(Bt, (long long)N * K * 2, "splitk Bt");
  hc::span(C, mn * 2, "splitk C");
  hc::span(workspace, std::min(workspace_elems, (long long)splits * mn) * 4, "splitk workspace");
  if (epi == 1 || epi == 2 || epi == 6) hc::span(bias, (long long)N * 4, "splitk bias");
  if (epi == 2 || epi == 3) hc::span(aux, mn * 2, "splitk aux");
  hc::opt_span(aux_out, mn * 2, "splitk aux_out");
  if (epi == 4 || epi >= 6) hc::span(res, mn * 2, "splitk res");
  if (colsum) {
    if (colsum_blocks) *colsum_blocks = (M + 31) / 32;
    hc::span(colsum, (long long)((M + 31) / 32) * N * 4, "splitk colsum");
  }
  if (ln) {
    hc::span(ln->gamma, (long long)N * 4, "splitk gamma");
    hc::span(ln->mean, (long long)M * 4, "splitk mean");
    hc::span(ln->rstd, (long long)M * 4, "splitk rstd");
    if (epi == 7) {
      hc::span(ln->z, mn * 2, "splitk z");
      hc::span(ln->colpart, mn * 3 * 4, "splitk colpart");
      if (ln->thr) hc::span(ln->dx, mn * 2, "splitk dx");
    } else {
      hc::span(ln->beta, (long long)N * 4, "splitk beta");
      hc::opt_span(ln->z, mn * 2, "splitk z");
    }
    if (ln->thr) {
      hc::span(ln->seed_ptr, 4, "splitk seed");
      hc::opt_span(ln->row_map, (long long)M * 4, "splitk row_map");
    }
  }
  return splits;
}
int fd_gemm_ln(int bwd, const void* A, const void* Bt, void* C, int M, int N, int K, const float* bias,
               const void* res, int ldres, const FdLnEpi* ln, int cfg, int b_mn, hipStream_t) {
  ++hc::calls;
  (void)b_mn;  // (W [K][N] or W^T [N][K]: the same N * K elements)
  const int bm = cfg == 13 ? 64 : 128;
  const long long tm = (M + bm - 1) / bm, mn = (long long)M * N;
  hc::span(A, (long long)M * K * 2, "gemm_ln A");
  hc::span(Bt, (long long)N * K * 2, "gemm_ln Bt");
  hc::span(C, mn * 2, "gemm_ln C");
  hc::span(res, (long long)M * ldres * 2, "gemm_ln res");
  hc::span(ln->gamma, (long long)N * 4, "gemm_ln gamma");
  hc::span(ln->mean, (long long)M * 4, "gemm_ln mean");
  hc::span(ln->rstd, (long long)M * 4, "gemm_ln rstd");
  hc::span(ln->stats, tm * (N / 64) * 2 * bm * 8, "gemm_ln stats");
  hc::span(ln->cnt, 4, "gemm_ln cnt");
  hc::span(ln->err, 4, "gemm_ln err");
  if (ln->pf) hc::span(ln->pf, ln->pf_bytes, "gemm_ln prefetch");  // (loads one dword per 64 B inside it)
  if (ln->xbuf) {  // two-K-half tiles: pairs x 2 x 32 (128-row) / 64 KiB (256-row) of partials,
                   // pairs x 2 flag granules; the 256-row tiles' statistics rows
    const long long pairs = tm * (N / 128), tm256 = (M + 255) / 256;
    hc::span(ln->xbuf, std::max(pairs * 2 * 32768, tm256 * (N / 128) * 2 * 65536), "gemm_ln xbuf");
    hc::span(ln->xflag, pairs * 2 * 8, "gemm_ln xflag");
    hc::span(ln->stats, tm256 * (N / 64) * 2 * 256 * 8, "gemm_ln stats (256-row tiles)");
  }
  if (bwd) {
    hc::span(ln->z, mn * 2, "gemm_ln z");
    hc::span(ln->colpart, tm * 3 * N * 4, "gemm_ln colpart");
    if (ln->thr) hc::span(ln->dx, mn * 2, "gemm_ln dx");
  } else {
    hc::span(bias, (long long)N * 4, "gemm_ln bias");
    hc::span(ln->beta, (long long)N * 4, "gemm_ln beta");
    hc::opt_span(ln->z, mn * 2, "gemm_ln z");
  }
  if (ln->thr) {
    hc::span(ln->seed_ptr, 4, "gemm_ln seed");
    hc::opt_span(ln->row_map, (long long)M * 4, "gemm_ln row_map");
  }
  return (int)tm;
}
int fd_splitk_reduce_batched(int n, const float* const* slabs, float* const* outs, const long long* numel,
                             const int* splits, const int*, hipStream_t) {
  ++hc::calls;
  for (int i = 0; i < n; ++i) {
    hc::span(slabs[i], numel[i] * splits[i] * 4, "reduce slabs");
    hc::span(outs[i], numel[i] * 4, "reduce out");
  }
  return 0;
}
const char* fd_comm_last_error() { return ""; }
int fd_comm_load(const char*) { return 0; }
int fd_comm_unique_id_bytes() { return 128; }
int fd_comm_get_unique_id(void*) { return 0; }
int fd_comm_init(void**, int, int, const void*) { return 0; }
int fd_comm_destroy(void*) { return 0; }
int fd_comm_async_error(void*) { return 0; }
int fd_comm_wait(void*, hipStream_t, long long) { return 0; }
int fd_comm_abort(void*) { return 0; }
int fd_comm_allreduce(void*, const void*, void*, long long, int, int, hipStream_t) { return 0; }
int fd_comm_broadcast(void*, void*, long long, int, int, hipStream_t) { return 0; }
int fd_comm_allgather(void*, const void*, void*, long long, int, hipStream_t) { return 0; }
int fd_attn_fwd(const void* qkv, const float* kbias, void* ctx, float* lse, int B, int S, int H, const uint32_t* seed,
                uint32_t, uint32_t, float, const int* cu, int rows, uint64_t* dmask, int, void* cxc, void* xc,
                const void* xres, int Bp, int, hipStream_t) {
  ++hc::calls;
  const long long D = (long long)H * 64;
  hc::opt_span(cxc, (long long)Bp * D * 2, "attn cxc");
  hc::opt_span(xc, (long long)Bp * D * 2, "attn xc");
  hc::opt_span(xres, rows * D * 2, "attn xres");
  hc::opt_span(dmask, (long long)B * H * 256 * 8, "attn dmask");
  hc::span(qkv, rows * 3 * D * 2, "attn qkv");
  hc::span(ctx, rows * D * 2, "attn ctx");
  hc::span(lse, (long long)B * H * S * 4, "attn lse");
  hc::span(seed, 4, "attn seed");
  if (cu) hc::span(cu, (long long)(B + 1) * 4, "attn cu");
  else hc::span(kbias, (long long)B * S * 4, "attn kbias");
  return 0;
}
int fd_gemm_attn_fwd(const void* x, const void* w, const float* bias, void* qkv, int M, int K, const float* kbias,
                     void* ctx, float* lse, int B, int S, int H, const uint32_t* seed, uint32_t, uint32_t, float,
                     const int* cu, int rows, uint64_t* dmask, int, void* cxc, void* xc, const void* xres, int Bp,
                     uint64_t* flags, int nflags, const int* cnt, int, int* err, int, int, hipStream_t) {
  ++hc::calls;
  if (g_hc_pf) hc::span(g_hc_pf, g_hc_pf_bytes, "gemm_attn prefetch");
  g_hc_pf = nullptr;
  g_hc_pf_bytes = 0;
  const long long D = (long long)H * 64, N = 3 * D;
  hc::span(x, (long long)M * K * 2, "gemm_attn x");
  hc::span(w, N * K * 2, "gemm_attn w");
  hc::span(bias, N * 4, "gemm_attn bias");
  hc::span(qkv, (long long)M * N * 2, "gemm_attn qkv");
  const long long tiles = ((M + 127) / 128) * (N / 192);
  if (tiles > nflags) hc::violations.push_back("gemm_attn: more tiles than flags");
  hc::span(flags, tiles * 8, "gemm_attn flags");
  hc::span(cnt, 4, "gemm_attn cnt");
  hc::span(err, 4, "gemm_attn err");
  hc::opt_span(cxc, (long long)Bp * D * 2, "gemm_attn cxc");
  hc::opt_span(xc, (long long)Bp * D * 2, "gemm_attn xc");
  hc::opt_span(xres, rows * D * 2, "gemm_attn xres");
  hc::opt_span(dmask, (long long)B * H * 256 * 8, "gemm_attn dmask");
  hc::span(ctx, rows * D * 2, "gemm_attn ctx");
  hc::span(lse, (long long)B * H * S * 4, "gemm_attn lse");
  hc::span(seed, 4, "gemm_attn seed");
  if (cu) hc::span(cu, (long long)(B + 1) * 4, "gemm_attn cu");
  else hc::span(kbias, (long long)B * S * 4, "gemm_attn kbias");
  return 0;
}
int fd_attn_bwd_proj(const void* qkv, const float* kbias, const void* ctx, const float* lse, const void* dy,
                     const void* w, int M, int K, int, void* dqkv, int B, int S, int H, const uint32_t* seed,
                     uint32_t, uint32_t, float, const int* cu, int rows, const uint64_t* dmask, const void* dresc,
                     void* dres, int, hipStream_t) {
  ++hc::calls;
  const long long D = (long long)H * 64;
  hc::opt_span(dmask, (long long)B * H * 256 * 8, "attn bwd proj dmask");
  hc::span(qkv, rows * 3 * D * 2, "attn bwd proj qkv");
  hc::span(dqkv, rows * 3 * D * 2, "attn bwd proj dqkv");
  hc::span(ctx, rows * D * 2, "attn bwd proj ctx");
  hc::span(dy, (long long)M * K * 2, "attn bwd proj dy");
  hc::span(w, (long long)K * D * 2, "attn bwd proj w");
  hc::opt_span(dresc, (long long)M * D * 2, "attn bwd proj dresc");
  hc::opt_span(dres, rows * D * 2, "attn bwd proj dres");
  hc::span(lse, (long long)B * H * S * 4, "attn bwd proj lse");
  hc::span(seed, 4, "attn bwd proj seed");
  if (cu) hc::span(cu, (long long)(B + 1) * 4, "attn bwd proj cu");
  else hc::span(kbias, (long long)B * S * 4, "attn bwd proj kbias");
  return 0;
}
int fd_attn_bwd(const void* qkv, const float* kbias, const void* ctx, const float* lse, const void* dctx, float* delta,
                void* dqkv, int B, int S, int H, const uint32_t* seed, uint32_t, uint32_t, float, const int* cu,
                int rows, const uint64_t* dmask, int, const void* dresc, void* dres, int, hipStream_t) {
  ++hc::calls;
  const long long D = (long long)H * 64;
  hc::opt_span(dmask, (long long)B * H * 256 * 8, "attn bwd dmask");
  hc::span(qkv, rows * 3 * D * 2, "attn bwd qkv");
  hc::span(dqkv, rows * 3 * D * 2, "attn bwd dqkv");
  hc::span(ctx, rows * D * 2, "attn bwd ctx");
  // (compact [CLS] gradients: dctx / dresc hold >= B rows, dres the full layout)
  hc::span(dctx, (dres ? B : rows) * D * 2, "attn bwd dctx");
  hc::opt_span(dresc, (long long)B * D * 2, "attn bwd dresc");
  hc::opt_span(dres, rows * D * 2, "attn bwd dres");
  hc::span(lse, (long long)B * H * S * 4, "attn bwd lse");
  hc::span(delta, (long long)B * H * S * 4, "attn bwd delta");
  hc::span(seed, 4, "attn bwd seed");
  if (cu) hc::span(cu, (long long)(B + 1) * 4, "attn bwd cu");
  else hc::span(kbias, (long long)B * S * 4, "attn bwd kbias");
  return 0;
}
int fd_mask_to_bias(const void*, int, float*, long, hipStream_t) { ++hc::calls; return 0; }
int fd_ln_fwd(const void* x, const void* r, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
              int T, int D, float, const uint32_t* seed, uint32_t, uint32_t, float, const int* row_map, hipStream_t) {
  ++hc::calls;
  const long long n = (long long)T * D;
  hc::span(x, n * 2, "ln x");
  hc::opt_span(r, n * 2, "ln r");
  hc::span(y, n * 2, "ln y");
  hc::span(gamma, (long long)D * 4, "ln gamma");
  hc::span(beta, (long long)D * 4, "ln beta");
  hc::span(mean, (long long)T * 4, "ln mean");
  hc::span(rstd, (long long)T * 4, "ln rstd");
  hc::span(seed, 4, "ln seed");
  hc::opt_span(row_map, (long long)T * 4, "ln row_map");
  return 0;
}
int fd_ln_bwd(const void* dy, const void* x, const void* r, const float* gamma, const float* mean, const float* rstd,
              void* dz, void* dx, float* dgamma, float* dbeta, float* dbias, float* work, int T, int D,
              const uint32_t* seed, uint32_t, uint32_t, float, int, const int* row_map, int, int* nblk_out,
              int, hipStream_t) {
  ++hc::calls;
  const long long n = (long long)T * D;
  hc::span(dy, n * 2, "ln bwd dy");
  hc::span(x, n * 2, "ln bwd x");
  hc::opt_span(r, n * 2, "ln bwd r");
  hc::span(dz, n * 2, "ln bwd dz");
  hc::opt_span(dx, n * 2, "ln bwd dx");
  hc::span(gamma, (long long)D * 4, "ln bwd gamma");
  hc::span(mean, (long long)T * 4, "ln bwd mean");
  hc::span(rstd, (long long)T * 4, "ln bwd rstd");
  hc::opt_span(dgamma, (long long)D * 4, "ln bwd dgamma");
  hc::opt_span(dbeta, (long long)D * 4, "ln bwd dbeta");
  hc::opt_span(dbias, (long long)D * 4, "ln bwd dbias");
  const int blocks = std::min(512, (T + 7) / 8);  // the kernel's partial-sum grid (csrc/kernels/norm.hip)
  hc::span(work, (long long)blocks * 3 * D * 4, "ln bwd work");
  hc::span(seed, 4, "ln bwd seed");
  hc::opt_span(row_map, (long long)T * 4, "ln bwd row_map");
  if (nblk_out) *nblk_out = blocks;
  return 0;
}
int fd_emb_fwd(const void*, int, const void*, const void*, const float*, const float*, void*, float*, float*, int, int,
               int, float, const uint32_t*, uint32_t, uint32_t, float, const int*, int* ln_epoch,
               unsigned long long* ln_stats, long long ln_stats_n, long long* sorted, long long* perm, hipStream_t) {
  ++hc::calls;
  hc::opt_span(ln_epoch, 4, "emb ln_epoch");
  hc::opt_span(ln_stats, ln_stats_n * 8, "emb ln_stats");
  if ((sorted == nullptr) != (perm == nullptr)) hc::violations.push_back("emb_fwd: sorted without perm");
  return 0;
}
int fd_emb_bwd(const void* dy, const void*, int, const long long* sorted, const long long* perm, const void*,
               const void*, const float*, const float*, const float*, float* dword, float* dpos, float*, float*,
               float* dz, float* work, int T, int, int, int P, int V, int D, const uint32_t*, uint32_t, uint32_t, float,
               int, unsigned char* now, unsigned char* ever, const int*, const int*, int ncs,
               const float* const* cs_parts, float* const* cs_outs, const int* cs_nblk, const int* cs_stride,
               const int* cs_D, const int* cs_nout, const int*, hipStream_t) {
  ++hc::calls;
  if (ncs < 0 || ncs > 32) hc::violations.push_back("emb_bwd: column-sum job count");
  for (int i = 0; i < ncs; ++i) {
    hc::span(cs_parts[i], (long long)cs_nblk[i] * cs_stride[i] * 4, "emb_bwd colsum part");
    for (int k = 0; k < cs_nout[i]; ++k) hc::opt_span(cs_outs[3 * i + k], (long long)cs_D[i] * 4, "emb_bwd colsum out");
  }
  hc::span(dy, (long long)T * D * 2, "emb_bwd dy");
  hc::span(sorted, (long long)T * 8, "emb_bwd sorted");
  hc::span(perm, (long long)T * 8, "emb_bwd perm");
  hc::span(dz, (long long)T * D * 4, "emb_bwd dz");
  // word-gradient pieces [T][D], then the LayerNorm partials [min(256, ceil(T / 8))][3][D]
  hc::span(work, ((long long)T * D + (long long)std::min(256, (T + 7) / 8) * 3 * D) * 4, "emb_bwd work");
  hc::span(dword, (long long)V * D * 4, "emb_bwd dword");
  hc::span(dpos, (long long)P * D * 4, "emb_bwd dpos");
  hc::opt_span(now, V, "emb_bwd now");
  hc::opt_span(ever, V, "emb_bwd ever");
  return 0;
}
int fd_gather_rows2(const void* a, const void* b, void* oa, void* ob, const long long* idx, int n, int d_bytes,
                    hipStream_t) {
  ++hc::calls;
  hc::span(oa, (long long)n * d_bytes, "gather_rows2 oa");
  hc::span(ob, (long long)n * d_bytes, "gather_rows2 ob");
  hc::span(idx, (long long)n * 8, "gather_rows2 idx");
  (void)a; (void)b;  // rows named by device indices
  return 0;
}
int fd_scatter_rows2(const void* a, const void* b, void* oa, void* ob, const long long* idx, int nsrc, int T,
                     int d_bytes, hipStream_t) {
  ++hc::calls;
  hc::span(a, (long long)nsrc * d_bytes, "scatter_rows2 a");
  hc::span(b, (long long)nsrc * d_bytes, "scatter_rows2 b");
  hc::span(oa, (long long)T * d_bytes, "scatter_rows2 oa");
  hc::span(ob, (long long)T * d_bytes, "scatter_rows2 ob");
  hc::span(idx, (long long)nsrc * 8, "scatter_rows2 idx");
  return 0;
}
int fd_pack(const void* mask, int mask_bytes, const void* ids, int ids_bytes, int B, int S, int rows, int* row_map,
            int* cu, long long* ids_packed, int* step, uint32_t* seed, long long* cls_rows, int* cls_rmap,
            hipStream_t) {
  hc::opt_span(cls_rmap, (long long)B * 4, "pack cls_rmap");
  ++hc::calls;
  hc::opt_span(cls_rows, (long long)B * 8, "pack cls_rows");
  hc::opt_span(step, 4, "pack step");
  hc::opt_span(seed, 4, "pack seed");
  hc::span(mask, (long long)B * S * mask_bytes, "pack mask");
  hc::span(ids, (long long)B * S * ids_bytes, "pack ids");
  hc::span(row_map, (long long)rows * 4, "pack row_map");
  hc::span(cu, (long long)(B + 1) * 4, "pack cu");
  hc::span(ids_packed, (long long)rows * 8, "pack ids_packed");
  return 0;
}
int fd_colsum_bf16(const void*, int, int, float*, float*, int, int, int* nblk_out, hipStream_t) {
  ++hc::calls;
  if (nblk_out) *nblk_out = 1;
  return 0;
}
int fd_colsum_bf16_batched(int n, const void* const* xs, const int* T, const int* N, float* const* parts,
                           hipStream_t) {
  ++hc::calls;
  for (int i = 0; i < n; ++i) {
    hc::span(xs[i], (long long)T[i] * N[i] * 2, "colsum_bf16_batched x");
    hc::span(parts[i], (long long)((T[i] + 31) / 32) * N[i] * 4, "colsum_bf16_batched part");
  }
  return 0;
}
int fd_colsum_batched(int, const float* const*, float* const*, const int*, const int*, const int*, const int*,
                      const int*, hipStream_t) { ++hc::calls; return 0; }
int fd_rank_sort(const void*, int, int, long long*, long long*, hipStream_t) { ++hc::calls; return 0; }
int fd_head_fwd(const void* hidden, int B, int S, int D, const float* W, const float* bias, const uint32_t* seed,
                uint32_t, uint32_t, float, const long long* labels, float* logits, float* loss, float* dlogits,
                float* row_loss, const int* cls, int T, const float* tlogits, float, float, float* loss_acc,
                hipStream_t) {
  ++hc::calls;
  hc::opt_span(loss_acc, 4, "head loss_acc");
  hc::span(hidden, (long long)T * D * 2, "head hidden");
  hc::span(W, 2LL * D * 4, "head W");
  hc::span(bias, 8, "head bias");
  hc::span(logits, 2LL * B * 4, "head logits");
  if (!cls && (long long)B * S > T) hc::violations.push_back("head: padded rows beyond hidden");
  hc::opt_span(cls, (long long)B * 4, "head cls");
  if (labels) {
    hc::span(labels, (long long)B * 8, "head labels");
    hc::span(loss, 4, "head loss");
    hc::span(dlogits, 2LL * B * 4, "head dlogits");
    hc::span(row_loss, (long long)B * 4, "head row_loss");
  }
  hc::opt_span(tlogits, 2LL * B * 4, "head teacher logits");
  hc::span(seed, 4, "head seed");
  return 0;
}
int fd_head_bwd(const void* hidden, int B, int S, int D, const float* W, const uint32_t* seed, uint32_t, uint32_t,
                float, const float* dlogits, float* dW, float* db, void* dhidden, int, const int* cls, int T,
                const float* gscale, const int* own, hipStream_t) {
  ++hc::calls;
  hc::opt_span(own, (B + 1LL) * 4, "head bwd own");
  hc::span(hidden, (long long)T * D * 2, "head bwd hidden");
  hc::span(dhidden, (long long)T * D * 2, "head bwd dhidden");
  hc::span(W, 2LL * D * 4, "head bwd W");
  hc::span(dlogits, 2LL * B * 4, "head bwd dlogits");
  hc::span(dW, 2LL * D * 4, "head bwd dW");
  hc::span(db, 8, "head bwd db");
  hc::opt_span(cls, (long long)B * 4, "head bwd cls");
  hc::opt_span(gscale, 4, "head bwd gscale");
  hc::span(seed, 4, "head bwd seed");
  (void)S;
  return 0;
}
int fd_head_ln_bwd(const void* hidden, int B, int T, int D, const float* W, const float* bias, const uint32_t* seed,
                   uint32_t, uint32_t, float, const long long* labels, float* logits, float* loss, float* dlogits,
                   float* row_loss, float* loss_acc, float* dW, float* db, int, const int* own, const float* tlogits,
                   float, float, const void* z, const float* gamma, const float* mean, const float* rstd, void* dz,
                   void* dx, float* part, uint32_t, uint32_t thr, float, const int* row_map, int* nblk_out,
                   hipStream_t) {
  ++hc::calls;
  const long long td = (long long)T * D;
  if (B > T) hc::violations.push_back("head_ln_bwd: B > T");
  hc::span(hidden, td * 2, "head_ln hidden");
  hc::span(W, 2LL * D * 4, "head_ln W");
  hc::span(bias, 8, "head_ln bias");
  hc::span(labels, (long long)B * 8, "head_ln labels");
  hc::span(logits, 2LL * B * 4, "head_ln logits");
  hc::span(loss, 4, "head_ln loss");
  hc::span(dlogits, 2LL * B * 4, "head_ln dlogits");
  hc::span(row_loss, (long long)B * 4, "head_ln row_loss");
  hc::opt_span(loss_acc, 4, "head_ln loss_acc");
  hc::span(dW, 2LL * D * 4, "head_ln dW");
  hc::span(db, 8, "head_ln db");
  hc::opt_span(own, (B + 1LL) * 4, "head_ln own");
  hc::opt_span(tlogits, 2LL * B * 4, "head_ln teacher logits");
  hc::span(z, td * 2, "head_ln z");
  hc::span(gamma, (long long)D * 4, "head_ln gamma");
  hc::span(mean, (long long)T * 4, "head_ln mean");
  hc::span(rstd, (long long)T * 4, "head_ln rstd");
  hc::span(dz, td * 2, "head_ln dz");
  if (thr) hc::span(dx, td * 2, "head_ln dx");
  const int nlb = (T + 15) / 16;
  hc::span(part, (long long)nlb * 3 * D * 4, "head_ln part");
  hc::opt_span(row_map, (long long)T * 4, "head_ln row_map");
  hc::span(seed, 4, "head_ln seed");
  if (nblk_out) *nblk_out = nlb;
  return 0;
}
int fd_eval_metrics(const float*, const long long*, int, double*, long long*, float*, long long*, hipStream_t) {
  ++hc::calls;
  return 0;
}
int fd_adam(float* p, const float* g, float* m, float* v, void* shadow, long long n, const int* step,
            const FdAdamHyper* h, const unsigned char* touched, const unsigned char* now, long long skip_off,
            long long skip_rows, int row_len, const long long* runs, int nruns, long long run_total4,
            const float* run_wd, const float* anchor, hipStream_t) {
  ++hc::calls;
  hc::hyper(h, "adam");
  if (h && h->mu != 0.f) hc::span(anchor, n * 4, "adam anchor");
  if (run_wd) {
    if (!runs) hc::violations.push_back("adam: run decays without a run table");
    hc::span(run_wd, (long long)nruns * 4, "adam run decays");
  }
  hc::span(p, n * 4, "adam p");
  hc::span(g, n * 4, "adam g");
  hc::span(m, n * 4, "adam m");
  hc::span(v, n * 4, "adam v");
  hc::opt_span(shadow, n * 2, "adam shadow");
  hc::span(step, 4, "adam step");
  if (touched) {
    hc::span(touched, skip_rows, "adam touched");
    hc::opt_span(now, skip_rows, "adam now");
    if (skip_off < 0 || skip_off + skip_rows * row_len > n) hc::violations.push_back("adam: skip range");
  }
  if (runs) {  // the kernel indexes [start4, start4 + count4) of every run (csrc/kernels/head_optim.hip)
    hc::span(runs, (long long)nruns * 3 * 8, "adam runs");
    long long pre = 0;
    for (int i = 0; i < nruns; ++i) {
      const long long s4 = runs[3 * i], c4 = runs[3 * i + 1], p4 = runs[3 * i + 2];
      if (s4 < 0 || c4 <= 0 || (s4 + c4) * 4 > n) hc::violations.push_back("adam: run outside the arena");
      if (p4 != pre) hc::violations.push_back("adam: run prefix");
      pre += c4;
    }
    if (pre != run_total4) hc::violations.push_back("adam: run total");
  }
  return 0;
}
int fd_lr_schedule_table(float* out, int n, float lr, const FdLrSched* sched, hipStream_t) {
  ++hc::calls;
  if (!sched) hc::violations.push_back("lr table: no schedule");
  else if (fd_lr_sched_rc(sched)) hc::violations.push_back("lr table: learning-rate schedule out of range");
  if (!std::isfinite(lr)) hc::violations.push_back("lr table: lr");
  hc::span(out, (long long)n * 4, "lr table out");
  return 0;
}
int fd_step(int*, uint32_t*, hipStream_t) { ++hc::calls; return 0; }
int fd_scale_cast(float*, void*, long long, float, hipStream_t) { ++hc::calls; return 0; }
int fd_axpby(float*, const float*, const float*, float, float, long long, hipStream_t) { ++hc::calls; return 0; }
// (the kernel's grid: ceil(n / 4 / 256) blocks, at most 4096 -- csrc/kernels/head_optim.hip grid_for)
int fd_server_opt_grid(long long n) { return n > 0 ? (int)std::min<long long>((n / 4 + 255) / 256, 4096) : 0; }
int fd_server_opt(float* master, float* x, float* m, float* v, void* shadow, long long n, int kind, float inv,
                  float eta, float b1, float b2, float tau, float* stats, hipStream_t) {
  ++hc::calls;
  // the kernel walks n / 4 float4 of every stream it is given, and writes 2 floats per block of stats
  if (n <= 0 || n % 4 != 0) hc::violations.push_back("server_opt: n % 4");
  if (kind < 0 || kind > 3) hc::violations.push_back("server_opt: kind");
  hc::span(master, n * 4, "server_opt master");
  hc::span(x, n * 4, "server_opt x");
  hc::span(m, n * 4, "server_opt m");
  if (kind != 0) hc::span(v, n * 4, "server_opt v");
  else if (v) hc::violations.push_back("server_opt: v with avgm");
  hc::opt_span(shadow, n * 2, "server_opt shadow");
  hc::opt_span(stats, 2LL * fd_server_opt_grid(n) * 4, "server_opt stats");
  if (!std::isfinite(inv) || !(inv > 0.f) || !std::isfinite(eta) || !(eta > 0.f) || !std::isfinite(tau) ||
      !(tau > 0.f) || !(b1 >= 0.f && b1 <= 1.f) || !(b2 >= 0.f && b2 <= 1.f))
    hc::violations.push_back("server_opt: hyper-parameters out of range");
  return 0;
}
// (the grid of fd_server_opt -- csrc/kernels/robust_agg.hip ra_grid_for)
int fd_robust_agg_grid(long long n) { return fd_server_opt_grid(n); }
int fd_robust_agg(const float* const* src, int M, int k, float* out, void* shadow, int* counts, long long n,
                  hipStream_t) {
  ++hc::calls;
  // the kernel reads n / 4 float4 of each of the M sources, writes as many to out (and uint2 to the
  // shadow), and 17 ints per block of counts
  if (n <= 0 || n % 4 != 0) hc::violations.push_back("robust_agg: n % 4");
  if (M < 2 || M > 16) {
    hc::violations.push_back("robust_agg: M");
    return 0;
  }
  if (k < 0 || 2 * k >= M) hc::violations.push_back("robust_agg: k");
  hc::span(out, n * 4, "robust_agg out");
  hc::opt_span(shadow, n * 2, "robust_agg shadow");
  hc::opt_span(counts, 17LL * fd_robust_agg_grid(n) * 4, "robust_agg counts");
  if (!src) {
    hc::violations.push_back("robust_agg: no sources");
    return 0;
  }
  const auto overlaps = [](const void* a, long long ab, const void* b, long long bb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)bb && b0 < a0 + (uintptr_t)ab;
  };
  for (int s = 0; s < M; ++s) {
    hc::span(src[s], n * 4, "robust_agg source");
    if (src[s] && overlaps(src[s], n * 4, out, n * 4)) hc::violations.push_back("robust_agg: out overlaps a source");
    if (src[s] && shadow && overlaps(src[s], n * 4, shadow, n * 2))
      hc::violations.push_back("robust_agg: shadow overlaps a source");
  }
  return 0;
}
// (the grid of fd_server_opt -- csrc/kernels/robust_dist.hip rd_grid_for)
int fd_robust_dist_grid(long long n) { return fd_server_opt_grid(n); }
int fd_robust_pairdist(const float* const* src, int M, double* partial, long long n, hipStream_t) {
  ++hc::calls;
  // the kernel reads n / 4 float4 of each of the M sources and writes M (M - 1) / 2 doubles per block
  if (n <= 0 || n % 4 != 0) hc::violations.push_back("robust_pairdist: n % 4");
  if (M < 2 || M > 16 || !src) {
    hc::violations.push_back("robust_pairdist: M");
    return 0;
  }
  for (int s = 0; s < M; ++s) hc::span(src[s], n * 4, "robust_pairdist source");
  hc::span(partial, 8LL * (M * (M - 1) / 2) * fd_robust_dist_grid(n), "robust_pairdist partial");
  return 0;
}
int fd_robust_krum_finalize(const double* partial, int grid, int M, int f, int m, float* ctl, double* stats,
                            hipStream_t) {
  ++hc::calls;
  // one block: reads grid rows of M (M - 1) / 2 doubles, writes 20 floats of ctl and 288 doubles of stats
  if (M < 2 || M > 16 || grid < 1 || grid > 4096) {
    hc::violations.push_back("robust_krum_finalize: M / grid");
    return 0;
  }
  if (f < 0 || m < 1 || m > M) hc::violations.push_back("robust_krum_finalize: f / m");
  hc::span(partial, 8LL * grid * (M * (M - 1) / 2), "robust_krum_finalize partial");
  hc::span(ctl, 20 * 4, "robust_krum_finalize ctl");
  hc::span(stats, 288 * 8, "robust_krum_finalize stats");
  return 0;
}
int fd_robust_wmean(const float* const* src, int M, const float* ctl, float* out, void* shadow, double* partial,
                    long long n, hipStream_t) {
  ++hc::calls;
  // the kernel reads 17 floats of ctl and n / 4 float4 of each source, writes as many to out (uint2 to
  // the shadow) and M + 1 doubles per block of partial
  if (n <= 0 || n % 4 != 0) hc::violations.push_back("robust_wmean: n % 4");
  if (M < 2 || M > 16 || !src) {
    hc::violations.push_back("robust_wmean: M");
    return 0;
  }
  hc::span(ctl, 20 * 4, "robust_wmean ctl");
  hc::opt_span(out, n * 4, "robust_wmean out");
  hc::opt_span(shadow, n * 2, "robust_wmean shadow");
  hc::opt_span(partial, 8LL * (M + 1) * fd_robust_dist_grid(n), "robust_wmean partial");
  if (shadow && !out) hc::violations.push_back("robust_wmean: shadow without out");
  const auto overlaps = [](const void* a, long long ab, const void* b, long long bb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)bb && b0 < a0 + (uintptr_t)ab;
  };
  for (int s = 0; s < M; ++s) {
    hc::span(src[s], n * 4, "robust_wmean source");
    if (src[s] && out && overlaps(src[s], n * 4, out, n * 4)) hc::violations.push_back("robust_wmean: out overlaps a source");
    if (src[s] && shadow && overlaps(src[s], n * 4, shadow, n * 2))
      hc::violations.push_back("robust_wmean: shadow overlaps a source");
  }
  return 0;
}
int fd_robust_geomed_finalize(const double* partial, int grid, int M, double nu, int iter, float* ctl, double* stats,
                              hipStream_t) {
  ++hc::calls;
  // one block: reads grid rows of M + 1 doubles, writes 20 floats of ctl and row iter (34 doubles) of stats
  if (M < 2 || M > 16 || grid < 1 || grid > 4096 || iter < 0) {
    hc::violations.push_back("robust_geomed_finalize: M / grid / iter");
    return 0;
  }
  if (!std::isfinite(nu) || !(nu > 0.0)) hc::violations.push_back("robust_geomed_finalize: nu");
  hc::span(partial, 8LL * grid * (M + 1), "robust_geomed_finalize partial");
  hc::span(ctl, 20 * 4, "robust_geomed_finalize ctl");
  hc::span(stats ? stats + 34LL * iter : nullptr, 34 * 8, "robust_geomed_finalize stats row");
  return 0;
}
// (the grid of fd_server_opt -- csrc/kernels/privacy.hip pv_grid_for)
int fd_privacy_grid(long long n) { return fd_server_opt_grid(n); }
namespace {
bool hc_overlaps(const void* a, long long ab, const void* b, long long bb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)bb && b0 < a0 + (uintptr_t)ab;
}
void hc_privacy_stream(long long round, long long client, long long first4, const char* what) {
  if (round < 0 || round > 0xffffffffll || client < 0 || client > 0xffffffffll || first4 < 0)
    hc::violations.push_back(std::string(what) + ": round / client / first4");
}
}  // namespace
int fd_privacy_norm(const float* w, const float* anchor, double* partial, float* stats, float clip, long long n,
                    hipStream_t) {
  ++hc::calls;
  // the kernels read n / 4 float4 of w and anchor, write one double per block of partial, and the
  // finalize reads those and writes the four floats of stats
  if (n <= 0 || n % 4 != 0) hc::violations.push_back("privacy_norm: n % 4");
  hc::span(w, n * 4, "privacy_norm w");
  hc::span(anchor, n * 4, "privacy_norm anchor");
  hc::span(partial, 8LL * fd_privacy_grid(n), "privacy_norm partial");
  hc::span(stats, 16, "privacy_norm stats");
  if (w && anchor && hc_overlaps(w, n * 4, anchor, n * 4)) hc::violations.push_back("privacy_norm: anchor overlaps w");
  if (!std::isfinite(clip) || !(clip > 0.f)) hc::violations.push_back("privacy_norm: clip");
  return 0;
}
int fd_privacy_apply(float* w, const float* anchor, void* shadow, const float* stats, float sigma, uint32_t, uint32_t,
                     long long round, long long client, long long first4, long long n, hipStream_t) {
  ++hc::calls;
  // the kernel reads stats[1..2], n / 4 float4 of w (and of anchor), writes as many to w and uint2 to
  // the shadow
  if (n <= 0 || n % 4 != 0) hc::violations.push_back("privacy_apply: n % 4");
  hc::span(w, n * 4, "privacy_apply w");
  hc::span(anchor, n * 4, "privacy_apply anchor");
  hc::opt_span(shadow, n * 2, "privacy_apply shadow");
  hc::span(stats, 16, "privacy_apply stats");
  if (w && anchor && hc_overlaps(w, n * 4, anchor, n * 4)) hc::violations.push_back("privacy_apply: anchor overlaps w");
  if (shadow && ((w && hc_overlaps(shadow, n * 2, w, n * 4)) || (anchor && hc_overlaps(shadow, n * 2, anchor, n * 4))))
    hc::violations.push_back("privacy_apply: shadow overlaps w or anchor");
  if (!std::isfinite(sigma) || !(sigma >= 0.f)) hc::violations.push_back("privacy_apply: sigma");
  hc_privacy_stream(round, client, first4, "privacy_apply");
  return 0;
}
int fd_privacy_gauss(float* out, uint32_t, uint32_t, long long round, long long client, long long first4, long long n,
                     hipStream_t) {
  ++hc::calls;
  if (n <= 0 || n % 4 != 0) hc::violations.push_back("privacy_gauss: n % 4");
  hc::span(out, n * 4, "privacy_gauss out");
  hc_privacy_stream(round, client, first4, "privacy_gauss");
  return 0;
}
// (the grid of fd_server_opt -- csrc/kernels/compress.hip qz_grid_for)
int fd_quant_grid(long long n) { return fd_server_opt_grid(n); }
long long fd_quant_words(long long n, int bits) {
  if (n <= 0 || n % 64 != 0 || (bits != 8 && bits != 4) || n > 0x3fffffffffffffffll / 8) return 0;
  return n * bits / 32 + n / 64;
}
int fd_quant_encode(const float* w, const float* anchor, float* residual, int32_t* payload, double* partial,
                    double* stats, int bits, int, uint32_t, uint32_t, long long round, long long client,
                    long long first, long long n, hipStream_t) {
  ++hc::calls;
  // the kernel reads n / 4 float4 of w, anchor (and residual, which it also writes), writes
  // fd_quant_words int32 of payload and three doubles per block of partial; the finalize reads those
  // and writes the four doubles of stats
  if (n <= 0 || n % 64 != 0) hc::violations.push_back("quant_encode: n % 64");
  if (bits != 8 && bits != 4) {
    hc::violations.push_back("quant_encode: bits");
    return 0;
  }
  const long long words = fd_quant_words(n, bits);
  hc::span(w, n * 4, "quant_encode w");
  hc::span(anchor, n * 4, "quant_encode anchor");
  hc::opt_span(residual, n * 4, "quant_encode residual");
  hc::span(payload, words * 4, "quant_encode payload");
  hc::span(partial, 3 * 8LL * fd_quant_grid(n), "quant_encode partial");
  hc::span(stats, 32, "quant_encode stats");
  const void* bufs[6] = {w, anchor, residual, payload, partial, stats};
  const long long bytes[6] = {n * 4, n * 4, n * 4, words * 4, 3 * 8LL * fd_quant_grid(n), 32};
  for (int i = 0; i < 6; ++i)
    for (int j = i + 1; j < 6; ++j)
      if (bufs[i] && bufs[j] && hc_overlaps(bufs[i], bytes[i], bufs[j], bytes[j]))
        hc::violations.push_back("quant_encode: buffers overlap");
  if (round < 0 || round > 0xffffffffll || client < 0 || client > 0xffffffffll || first < 0 ||
      first > (0x7fffffffffffffffll - n / 4) / 16)
    hc::violations.push_back("quant_encode: round / client / first");
  return 0;
}
int fd_quant_decode_mean(const int32_t* const* src, int M, const float* anchor, float* out, void* shadow, int bits,
                         long long n, hipStream_t) {
  ++hc::calls;
  // the kernel reads fd_quant_words int32 of each of the M payloads and n / 4 float4 of anchor, writes
  // as many float4 to out (and uint2 to the shadow)
  if (n <= 0 || n % 64 != 0) hc::violations.push_back("quant_decode_mean: n % 64");
  if (M < 1 || M > 16 || (bits != 8 && bits != 4)) {
    hc::violations.push_back("quant_decode_mean: M / bits");
    return 0;
  }
  const long long words = fd_quant_words(n, bits);
  hc::span(anchor, n * 4, "quant_decode_mean anchor");
  hc::span(out, n * 4, "quant_decode_mean out");
  hc::opt_span(shadow, n * 2, "quant_decode_mean shadow");
  if (anchor && out && hc_overlaps(anchor, n * 4, out, n * 4)) hc::violations.push_back("quant_decode_mean: out overlaps anchor");
  if (shadow && ((out && hc_overlaps(shadow, n * 2, out, n * 4)) || (anchor && hc_overlaps(shadow, n * 2, anchor, n * 4))))
    hc::violations.push_back("quant_decode_mean: shadow overlaps out or anchor");
  if (!src) {
    hc::violations.push_back("quant_decode_mean: no payloads");
    return 0;
  }
  for (int s = 0; s < M; ++s) {
    hc::span(src[s], words * 4, "quant_decode_mean payload");
    if (src[s] && ((out && hc_overlaps(src[s], words * 4, out, n * 4)) || (shadow && hc_overlaps(src[s], words * 4, shadow, n * 2))))
      hc::violations.push_back("quant_decode_mean: an output overlaps a payload");
  }
  return 0;
}
// (csrc/kernels/sparsify.hip: chunks of 4096 elements, at most 1024 blocks, the layout of `work`)
namespace {
bool hc_topk_n_ok(long long n) { return n > 0 && n % 64 == 0 && n <= 0x7fffffc0ll; }
long long hc_topk_chunks(long long n) { return (n + 4095) / 4096; }
}  // namespace
int fd_topk_grid(long long n) { return hc_topk_n_ok(n) ? (int)std::min<long long>(hc_topk_chunks(n), 1024) : 0; }
long long fd_topk_words(long long n, long long k) {
  if (!hc_topk_n_ok(n) || k < 1 || k > n / 2) return 0;
  return hc_topk_chunks(n) + 1 + k + (k + 1) / 2;
}
long long fd_topk_work_bytes(long long n) {
  if (!hc_topk_n_ok(n)) return 0;
  return n * 4 + (2048 + 1024 + 1024 + 16) * 4ll + hc_topk_chunks(n) * 16 + fd_topk_grid(n) * 16ll;
}
int fd_topk_encode(const float* w, const float* anchor, float* residual, int32_t* payload, void* work, double* stats,
                   long long k, long long n, hipStream_t) {
  ++hc::calls;
  // the kernels read n / 4 float4 of w, anchor (and residual, which they also write), write
  // fd_topk_words int32 of payload (the index halves as uint16: 2 * ceil(k / 2) of them), use
  // fd_topk_work_bytes of work from a 16-byte aligned base, and the finalize writes eight doubles of stats
  if (!hc_topk_n_ok(n)) {
    hc::violations.push_back("topk_encode: n % 64 / n < 2^31");
    return 0;
  }
  if (k < 1 || k > n / 2) {
    hc::violations.push_back("topk_encode: k");
    return 0;
  }
  const long long words = fd_topk_words(n, k), wbytes = fd_topk_work_bytes(n);
  hc::span(w, n * 4, "topk_encode w");
  hc::span(anchor, n * 4, "topk_encode anchor");
  hc::opt_span(residual, n * 4, "topk_encode residual");
  hc::span(payload, words * 4, "topk_encode payload");
  hc::span(work, wbytes, "topk_encode work");
  hc::span(stats, 64, "topk_encode stats");
  if (((uintptr_t)work & 15u) != 0) hc::violations.push_back("topk_encode: work alignment");
  const void* bufs[6] = {w, anchor, residual, payload, work, stats};
  const long long bytes[6] = {n * 4, n * 4, n * 4, words * 4, wbytes, 64};
  for (int i = 0; i < 6; ++i)
    for (int j = i + 1; j < 6; ++j)
      if (bufs[i] && bufs[j] && hc_overlaps(bufs[i], bytes[i], bufs[j], bytes[j]))
        hc::violations.push_back("topk_encode: buffers overlap");
  return 0;
}
int fd_topk_decode_mean(const int32_t* const* src, int M, const float* anchor, float* out, void* shadow, long long k,
                        long long n, hipStream_t) {
  ++hc::calls;
  // the kernel reads, of each of the M payloads, the C + 1 offsets and -- whatever they hold -- entries
  // in [0, k) only: k value words and ceil(k / 2) index words; n / 4 float4 of anchor; it writes as many
  // float4 to out (and uint2 to the shadow)
  if (!hc_topk_n_ok(n)) {
    hc::violations.push_back("topk_decode_mean: n % 64 / n < 2^31");
    return 0;
  }
  if (M < 1 || M > 16 || k < 1 || k > n / 2) {
    hc::violations.push_back("topk_decode_mean: M / k");
    return 0;
  }
  const long long words = fd_topk_words(n, k);
  hc::span(anchor, n * 4, "topk_decode_mean anchor");
  hc::span(out, n * 4, "topk_decode_mean out");
  hc::opt_span(shadow, n * 2, "topk_decode_mean shadow");
  if (anchor && out && hc_overlaps(anchor, n * 4, out, n * 4)) hc::violations.push_back("topk_decode_mean: out overlaps anchor");
  if (shadow && ((out && hc_overlaps(shadow, n * 2, out, n * 4)) || (anchor && hc_overlaps(shadow, n * 2, anchor, n * 4))))
    hc::violations.push_back("topk_decode_mean: shadow overlaps out or anchor");
  if (!src) {
    hc::violations.push_back("topk_decode_mean: no payloads");
    return 0;
  }
  for (int s = 0; s < M; ++s) {
    hc::span(src[s], words * 4, "topk_decode_mean payload");
    if (src[s] && ((out && hc_overlaps(src[s], words * 4, out, n * 4)) || (shadow && hc_overlaps(src[s], words * 4, shadow, n * 2))))
      hc::violations.push_back("topk_decode_mean: an output overlaps a payload");
  }
  return 0;
}
// (csrc/kernels/secagg.hip: one lane per float4, the check block's four behind the tensor, at most 2048 blocks)
namespace {
bool hc_secagg_n_ok(long long n) { return n > 0 && n % 16 == 0 && n <= 0x3fffffffffffffffll / 8; }
bool hc_secagg_blocks_ok(long long first_block, long long n, int extra) {
  return first_block >= 0 && first_block <= 0x100000000ll && first_block + n / 16 + extra <= 0x100000000ll;
}
}  // namespace
int fd_secagg_grid(long long n) { return n > 0 ? (int)std::min<long long>((n / 4 + 4 + 255) / 256, 2048) : 0; }
long long fd_secagg_words(long long n) { return hc_secagg_n_ok(n) ? n + 16 : 0; }
int fd_secagg_stream(int32_t* out, const uint32_t* key, uint32_t, uint32_t, uint32_t, int rounds, long long first_block,
                     long long n, hipStream_t) {
  ++hc::calls;
  // the kernel reads the 8 key words and writes n / 4 uint4 of out
  if (!hc_secagg_n_ok(n)) {
    hc::violations.push_back("secagg_stream: n % 16");
    return 0;
  }
  hc::span(out, n * 4, "secagg_stream out");
  hc::span(key, 32, "secagg_stream key");
  if (((uintptr_t)out & 15u) != 0) hc::violations.push_back("secagg_stream: out alignment");
  if (out && key && hc_overlaps(out, n * 4, key, 32)) hc::violations.push_back("secagg_stream: out overlaps key");
  if (rounds != 8 && rounds != 12 && rounds != 20) hc::violations.push_back("secagg_stream: rounds");
  if (!hc_secagg_blocks_ok(first_block, n, 0)) hc::violations.push_back("secagg_stream: first_block");
  return 0;
}
int fd_secagg_mask(const float* w, const float* anchor, const uint32_t* keys, int P, uint32_t signs, int32_t* payload,
                   double* partial, double* stats, int frac_bits, int rounds, long long round, long long first_block,
                   long long n, hipStream_t) {
  ++hc::calls;
  // the kernel reads n / 4 float4 of w and anchor and 8 * P key words, writes n / 4 + 4 uint4 of payload
  // and four doubles per block of partial; the finalize reads those and writes the four doubles of stats
  if (!hc_secagg_n_ok(n)) {
    hc::violations.push_back("secagg_mask: n % 16");
    return 0;
  }
  if (P < 0 || P > 15 || (signs >> P) != 0u) {
    hc::violations.push_back("secagg_mask: P / signs");
    return 0;
  }
  const long long grid = fd_secagg_grid(n);
  hc::span(w, n * 4, "secagg_mask w");
  hc::span(anchor, n * 4, "secagg_mask anchor");
  if (P > 0) hc::span(keys, 32LL * P, "secagg_mask keys");
  hc::span(payload, (n + 16) * 4, "secagg_mask payload");
  hc::span(partial, 4 * 8LL * grid, "secagg_mask partial");
  hc::span(stats, 32, "secagg_mask stats");
  if ((((uintptr_t)w | (uintptr_t)anchor | (uintptr_t)payload) & 15u) != 0)
    hc::violations.push_back("secagg_mask: alignment");
  const void* bufs[6] = {w, anchor, payload, partial, stats, P > 0 ? keys : nullptr};
  const long long bytes[6] = {n * 4, n * 4, (n + 16) * 4, 4 * 8LL * grid, 32, 32LL * P};
  for (int i = 0; i < 6; ++i)
    for (int j = i + 1; j < 6; ++j)
      if (bufs[i] && bufs[j] && hc_overlaps(bufs[i], bytes[i], bufs[j], bytes[j]))
        hc::violations.push_back("secagg_mask: buffers overlap");
  if (frac_bits < 8 || frac_bits > 30) hc::violations.push_back("secagg_mask: frac_bits");
  if (rounds != 8 && rounds != 12 && rounds != 20) hc::violations.push_back("secagg_mask: rounds");
  if (round < 0 || round > 0xffffffffll || !hc_secagg_blocks_ok(first_block, n, 1))
    hc::violations.push_back("secagg_mask: round / first_block");
  return 0;
}
int fd_secagg_unmask_mean(const int32_t* const* src, int M, const float* anchor, float* out, void* shadow,
                          int frac_bits, long long n, hipStream_t) {
  ++hc::calls;
  // the kernel reads n / 4 uint4 of each of the M payloads (which hold n + 16 words) and as many float4
  // of anchor, writes as many float4 to out (and uint2 to the shadow)
  if (!hc_secagg_n_ok(n)) {
    hc::violations.push_back("secagg_unmask_mean: n % 16");
    return 0;
  }
  if (M < 1 || M > 16 || frac_bits < 8 || frac_bits > 30) {
    hc::violations.push_back("secagg_unmask_mean: M / frac_bits");
    return 0;
  }
  hc::span(anchor, n * 4, "secagg_unmask_mean anchor");
  hc::span(out, n * 4, "secagg_unmask_mean out");
  hc::opt_span(shadow, n * 2, "secagg_unmask_mean shadow");
  if ((((uintptr_t)anchor | (uintptr_t)out) & 15u) != 0 || ((uintptr_t)shadow & 7u) != 0)
    hc::violations.push_back("secagg_unmask_mean: alignment");
  if (anchor && out && hc_overlaps(anchor, n * 4, out, n * 4)) hc::violations.push_back("secagg_unmask_mean: out overlaps anchor");
  if (shadow && ((out && hc_overlaps(shadow, n * 2, out, n * 4)) || (anchor && hc_overlaps(shadow, n * 2, anchor, n * 4))))
    hc::violations.push_back("secagg_unmask_mean: shadow overlaps out or anchor");
  if (!src) {
    hc::violations.push_back("secagg_unmask_mean: no payloads");
    return 0;
  }
  for (int s = 0; s < M; ++s) {
    hc::span(src[s], (n + 16) * 4, "secagg_unmask_mean payload");
    if (((uintptr_t)src[s] & 15u) != 0) hc::violations.push_back("secagg_unmask_mean: payload alignment");
    if (src[s] && ((out && hc_overlaps(src[s], (n + 16) * 4, out, n * 4)) ||
                   (shadow && hc_overlaps(src[s], (n + 16) * 4, shadow, n * 2))))
      hc::violations.push_back("secagg_unmask_mean: an output overlaps a payload");
  }
  return 0;
}
}  // extern "C"

// ------------------------------------------------------------------ driver
namespace {
int failures = 0;

at::Tensor T_(at::IntArrayRef shape, at::ScalarType dt) {
  at::Tensor t = at::zeros(shape, at::TensorOptions().dtype(dt));
  hc::reg(t);
  return t;
}

template <typename F>
void expect_ok(const char* name, F f) {
  const size_t v0 = hc::violations.size();
  const int c0 = hc::calls;
  try {
    f();
  } catch (const c10::Error& e) {
    std::printf("FAIL %s: unexpected rejection: %s\n", name, e.what_without_backtrace());
    ++failures;
    return;
  }
  if (hc::calls == c0) {
    std::printf("FAIL %s: no launcher was called\n", name);
    ++failures;
  }
  for (size_t i = v0; i < hc::violations.size(); ++i) {
    std::printf("FAIL %s: %s\n", name, hc::violations[i].c_str());
    ++failures;
  }
}

template <typename F>
void expect_reject(const char* name, F f) {
  const int c0 = hc::calls;
  bool threw = false;
  try {
    f();
  } catch (const c10::Error&) {
    threw = true;
  }
  if (!threw) {
    std::printf("FAIL %s: accepted a call the kernels do not support\n", name);
    ++failures;
  } else if (hc::calls != c0) {
    std::printf("FAIL %s: rejected only after launching\n", name);
    ++failures;
  }
}

const c10::optional<at::Tensor> none = c10::nullopt;
}  // namespace

int main() {
  const auto bf = at::kBFloat16, f32 = at::kFloat, i32 = at::kInt, i64 = at::kLong;
  // ---- GEMMs: y = x W^T + b (NT), dx = dy W (NN), dW (TN); the DistilBERT shapes at a packed bs32 step
  {
    auto x = T_({2688, 768}, bf), w = T_({2304, 768}, bf), y = T_({2688, 2304}, bf), b = T_({2304}, f32);
    expect_ok("gemm NT bias", [&] { gemm(0, 1, x, w, y, b, none, none, none, false, none); });
    auto w1 = T_({3072, 768}, bf), g = T_({2688, 3072}, bf), u = T_({2688, 3072}, bf), b1 = T_({3072}, f32);
    expect_ok("gemm NT bias+gelu", [&] { gemm(0, 2, x, w1, g, b1, u, none, none, false, none); });
    auto dy = T_({2688, 768}, bf), w2t = T_({3072, 768}, bf), du = T_({2688, 3072}, bf), gout = T_({2688, 3072}, bf);
    expect_ok("gemm NT gelu' + remat", [&] { gemm(0, 3, dy, w2t, du, none, u, none, none, false, gout); });
    auto res = T_({2688, 768}, bf), wt = T_({768, 3072}, bf), dx = T_({2688, 768}, bf);
    expect_ok("gemm NT residual", [&] { gemm(0, 4, du, wt, dx, none, none, res, none, false, none); });
    auto w2 = T_({768, 3072}, bf);
    expect_ok("gemm NN", [&] { gemm(1, 0, dy, w2, du, none, none, none, none, false, none); });
    auto dW = T_({2304, 768}, f32), dq = T_({2688, 2304}, bf), ws = T_({8 * 2304 * 768}, f32);
    expect_ok("gemm TN", [&] { gemm(2, 5, dq, x, dW, none, none, none, ws, false, none); });
    auto cs = T_({21 * 3072}, f32);
    expect_ok("gemm colsum", [&] { gemm_colsum(3, dy, w2t, du, u, none, cs, gout); });
    // rejections
    auto xk = T_({2688, 700}, bf), wk = T_({2304, 700}, bf);
    expect_reject("gemm K % 64", [&] { gemm(0, 1, xk, wk, y, b, none, none, none, false, none); });
    expect_reject("gemm C shape", [&] { gemm(0, 1, x, w, dx, b, none, none, none, false, none); });
    expect_reject("gemm bias size", [&] { gemm(0, 1, x, w, y, b1, none, none, none, false, none); });
    auto xf = T_({2688, 768}, f32);
    expect_reject("gemm dtype", [&] { gemm(0, 1, xf, w, y, b, none, none, none, false, none); });
    // (bias+GELU without u: a forward without autograd keeps only the activation)
    expect_ok("gemm NT bias+gelu, no u", [&] { gemm(0, 2, x, w1, g, b1, none, none, none, false, none); });
    expect_reject("gemm aux missing", [&] { gemm(0, 3, dy, w2t, du, none, none, none, none, false, none); });
    expect_reject("gemm aux shape", [&] { gemm(0, 2, x, w1, g, b1, y, none, none, false, none); });
    expect_reject("gemm aux_out epi", [&] { gemm(0, 1, x, w, y, b, none, none, none, false, gout); });
    auto xt = x.t();
    expect_reject("gemm non-contiguous", [&] { gemm(0, 1, xt, w, y, b, none, none, none, false, none); });
    auto cs_small = T_({3072}, f32);
    expect_reject("gemm colsum size", [&] { gemm_colsum(3, dy, w2t, du, u, none, cs_small, gout); });
    // batched bf16 column-sum partials (per-layer qkv-bias partials at the end of the backward)
    auto p1 = T_({84 * 2304}, f32), p2 = T_({84 * 3072}, f32), p_small = T_({83 * 2304}, f32);
    expect_ok("colsum_bf16_batched", [&] { colsum_bf16_batched({dq, du}, {p1, p2}, {2304, 3072}); });
    expect_reject("colsum_bf16_batched part size", [&] { colsum_bf16_batched({dq}, {p_small}, {2304}); });
    expect_reject("colsum_bf16_batched N", [&] { colsum_bf16_batched({dq}, {p1}, {2303}); });
    expect_reject("colsum_bf16_batched dtype", [&] { colsum_bf16_batched({p1}, {p1}, {2304}); });
  }
  // ---- all-layer weight gradients (with and without the fused Adam epilogue)
  {
    std::vector<at::Tensor> As, Bs, Cs, st;
    const int64_t shapes[4][2] = {{2304, 768}, {768, 768}, {3072, 768}, {768, 3072}};
    for (auto& sh : shapes) {
      As.push_back(T_({2688, sh[0]}, bf));
      Bs.push_back(T_({2688, sh[1]}, bf));
      Cs.push_back(T_({sh[0], sh[1]}, f32));
      st.push_back(T_({sh[0] * sh[1]}, f32));
      st.push_back(T_({sh[0] * sh[1]}, f32));
      st.push_back(T_({sh[0] * sh[1]}, f32));
      st.push_back(T_({sh[0] * sh[1]}, bf));
    }
    st.push_back(T_({1}, i32));
    const std::vector<double> hp = {2e-5, 0.9, 0.999, 1e-8, 0.0, 0.0};
    std::vector<int64_t> acc(4, 0), acc1 = {0, 1, 0, 0};
    expect_ok("dw_batch", [&] { gemm_dw_batch(As, Bs, Cs, acc, {}, {}, -1); });
    expect_ok("dw_batch adam", [&] { gemm_dw_batch(As, Bs, Cs, acc, st, hp, -1); });
    expect_reject("dw_batch adam+accumulate", [&] { gemm_dw_batch(As, Bs, Cs, acc1, st, hp, -1); });
    // parameter groups: a weight decay per problem (and per in-launch bias)
    const std::vector<double> hpw = {2e-5, 0.9, 0.999, 1e-8, 0.01, 1.0};
    expect_ok("dw_batch decays", [&] { gemm_dw_batch(As, Bs, Cs, acc, st, hpw, -1, {}, {}, {}, {0.01, 0.0, 0.01, 0.0}); });
    expect_reject("dw_batch decays length", [&] { gemm_dw_batch(As, Bs, Cs, acc, st, hpw, -1, {}, {}, {}, {0.01, 0.0}); });
    expect_reject("dw_batch decay negative", [&] {
      gemm_dw_batch(As, Bs, Cs, acc, st, hpw, -1, {}, {}, {}, {0.01, 0.0, -1.0, 0.0}); });
    expect_reject("dw_batch decay inf", [&] {
      gemm_dw_batch(As, Bs, Cs, acc, st, hpw, -1, {}, {}, {}, {0.01, 0.0, INFINITY, 0.0}); });
    expect_reject("dw_batch bias decays length", [&] {
      gemm_dw_batch(As, Bs, Cs, acc, st, hpw, -1, {}, {}, {}, {}, {0.0}); });
    expect_reject("dw_batch decays without adam", [&] {
      gemm_dw_batch(As, Bs, Cs, acc, {}, {}, -1, {}, {}, {}, {0.01, 0.0, 0.01, 0.0}); });
    {  // the rest of the step in the launch: per-run decays and the word table's decay
      const int64_t an = 64 * 64 + 1024;
      std::vector<at::Tensor> rest = {T_({an}, f32), T_({an}, f32), T_({an}, f32), T_({an}, f32), T_({an}, bf),
                                      T_({2, 3}, i64), T_({64}, at::kByte), T_({64}, at::kByte)};
      auto rp = rest[5].data_ptr<int64_t>();
      rp[0] = 1024; rp[1] = 128; rp[2] = 0; rp[3] = 1152; rp[4] = 128; rp[5] = 128;
      const std::vector<int64_t> ri = {256, 0, 64, 64};
      const c10::optional<at::Tensor> rw = T_({2}, f32), rw1 = T_({1}, f32);
      expect_ok("dw_batch rest", [&] { gemm_dw_batch(As, Bs, Cs, acc, st, hpw, -1, {}, rest, ri); });
      expect_ok("dw_batch rest decays", [&] {
        gemm_dw_batch(As, Bs, Cs, acc, st, hpw, -1, {}, rest, ri, {}, {}, rw, {0.01, 0.0}, 0.01); });
      expect_reject("dw_batch rest decays length", [&] {
        gemm_dw_batch(As, Bs, Cs, acc, st, hpw, -1, {}, rest, ri, {}, {}, rw1, {0.01}, 0.0); });
      expect_reject("dw_batch rest decays host", [&] {
        gemm_dw_batch(As, Bs, Cs, acc, st, hpw, -1, {}, rest, ri, {}, {}, rw, {0.01}, 0.0); });
      expect_reject("dw_batch rest decay negative", [&] {
        gemm_dw_batch(As, Bs, Cs, acc, st, hpw, -1, {}, rest, ri, {}, {}, rw, {0.01, -0.5}, 0.0); });
      expect_reject("dw_batch word decay coupled", [&] {
        gemm_dw_batch(As, Bs, Cs, acc, st, {2e-5, 0.9, 0.999, 1e-8, 0.01, 0.0}, -1, {}, rest, ri, {}, {}, none, {}, 0.01); });
      expect_reject("dw_batch word decay negative", [&] {
        gemm_dw_batch(As, Bs, Cs, acc, st, hpw, -1, {}, rest, ri, {}, {}, none, {}, -0.01); });
      expect_reject("dw_batch rest decays without rest", [&] {
        gemm_dw_batch(As, Bs, Cs, acc, st, hpw, -1, {}, {}, {}, {}, {}, rw, {0.01, 0.0}, 0.0); });
      // FedProx: an anchor per fused matrix, and the arena's with the rest of the step
      std::vector<at::Tensor> anc, anc_short;
      for (auto& sh : shapes) anc.push_back(T_({sh[0] * sh[1]}, f32));
      anc_short = anc;
      anc_short[2] = T_({3072 * 768 - 4}, f32);
      auto anc_rest = anc, anc_rest_short = anc;
      anc_rest.push_back(T_({an}, f32));
      anc_rest_short.push_back(T_({an - 4}, f32));
      expect_ok("dw_batch prox", [&] {
        gemm_dw_batch(As, Bs, Cs, acc, st, hpw, -1, {}, {}, {}, {}, {}, none, {}, 0.0, {}, 0.1, anc); });
      expect_ok("dw_batch prox rest", [&] {
        gemm_dw_batch(As, Bs, Cs, acc, st, hpw, -1, {}, rest, ri, {}, {}, none, {}, 0.0, {}, 0.1, anc_rest); });
      expect_ok("dw_batch prox mu 0", [&] {
        gemm_dw_batch(As, Bs, Cs, acc, st, hpw, -1, {}, rest, ri, {}, {}, none, {}, 0.0, {}, 0.0, anc_rest); });
      expect_reject("dw_batch prox no anchor", [&] {
        gemm_dw_batch(As, Bs, Cs, acc, st, hpw, -1, {}, {}, {}, {}, {}, none, {}, 0.0, {}, 0.1, {}); });
      expect_reject("dw_batch prox short anchor", [&] {
        gemm_dw_batch(As, Bs, Cs, acc, st, hpw, -1, {}, {}, {}, {}, {}, none, {}, 0.0, {}, 0.1, anc_short); });
      expect_reject("dw_batch prox rest without the arena's anchor", [&] {
        gemm_dw_batch(As, Bs, Cs, acc, st, hpw, -1, {}, rest, ri, {}, {}, none, {}, 0.0, {}, 0.1, anc); });
      expect_reject("dw_batch prox rest short anchor", [&] {
        gemm_dw_batch(As, Bs, Cs, acc, st, hpw, -1, {}, rest, ri, {}, {}, none, {}, 0.0, {}, 0.1, anc_rest_short); });
      expect_reject("dw_batch prox + decaying sparse word table", [&] {
        gemm_dw_batch(As, Bs, Cs, acc, st, hpw, -1, {}, rest, ri, {}, {}, none, {}, 0.01, {}, 0.1, anc_rest); });
      expect_reject("dw_batch prox without adam", [&] {
        gemm_dw_batch(As, Bs, Cs, acc, {}, {}, -1, {}, {}, {}, {}, {}, none, {}, 0.0, {}, 0.1, anc); });
      expect_reject("dw_batch prox mu negative", [&] {
        gemm_dw_batch(As, Bs, Cs, acc, st, hpw, -1, {}, {}, {}, {}, {}, none, {}, 0.0, {}, -0.1, anc); });
      expect_reject("dw_batch prox mu inf", [&] {
        gemm_dw_batch(As, Bs, Cs, acc, st, hpw, -1, {}, {}, {}, {}, {}, none, {}, 0.0, {}, INFINITY, anc); });
    }
    auto Bbad = Bs;
    Bbad[2] = T_({2000, 768}, bf);
    expect_ok("dw_batch sched", [&] { gemm_dw_batch(As, Bs, Cs, acc, st, hpw, -1, {}, {}, {}, {}, {}, none, {}, 0.0,
                                                    {1, 3, 10, 0}); });
    expect_reject("dw_batch sched kind", [&] { gemm_dw_batch(As, Bs, Cs, acc, st, hpw, -1, {}, {}, {}, {}, {}, none, {},
                                                             0.0, {3, 3, 10, 0}); });
    expect_reject("dw_batch sched warmup > total", [&] { gemm_dw_batch(As, Bs, Cs, acc, st, hpw, -1, {}, {}, {}, {}, {},
                                                                       none, {}, 0.0, {1, 11, 10, 0}); });
    expect_reject("dw_batch sched without adam", [&] { gemm_dw_batch(As, Bs, Cs, acc, {}, {}, -1, {}, {}, {}, {}, {},
                                                                     none, {}, 0.0, {1, 3, 10, 0}); });
    expect_reject("dw_batch lr inf", [&] { gemm_dw_batch(As, Bs, Cs, acc, st, {INFINITY, 0.9, 0.999, 1e-8, 0.0, 0.0},
                                                         -1); });
    expect_reject("dw_batch K mismatch", [&] { gemm_dw_batch(As, Bbad, Cs, acc, {}, {}, -1); });
    // per-problem rows (the pruned last block: padded [CLS] rows)
    auto Amix = As, Bmix = Bs;
    Amix[1] = T_({64, As[1].size(1)}, bf);
    Bmix[1] = T_({64, Bs[1].size(1)}, bf);
    expect_ok("dw_batch mixed K", [&] { gemm_dw_batch(Amix, Bmix, Cs, acc, st, hp, -1); });
    auto Bodd = Bmix;
    Bodd[1] = T_({96, Bs[1].size(1)}, bf);
    auto Aodd = Amix;
    Aodd[1] = T_({96, As[1].size(1)}, bf);
    expect_reject("dw_batch K % 64", [&] { gemm_dw_batch(Aodd, Bodd, Cs, acc, {}, {}, -1); });
    auto Cbad = Cs;
    Cbad[1] = T_({768, 3072}, f32);
    expect_reject("dw_batch C shape", [&] { gemm_dw_batch(As, Bs, Cbad, acc, {}, {}, -1); });
    auto stbad = st;
    stbad[5] = T_({100}, f32);
    expect_reject("dw_batch adam state size", [&] { gemm_dw_batch(As, Bs, Cs, acc, stbad, hp, -1); });
    std::vector<at::Tensor> A33(33, As[1]), B33(33, Bs[1]), C33(33, Cs[1]);
    expect_reject("dw_batch > 32 problems", [&] { gemm_dw_batch(A33, B33, C33, std::vector<int64_t>(33, 0), {}, {}, -1); });
    auto A0 = T_({2688, 768}, bf), B0 = T_({2688, 3072}, bf), C0 = T_({768, 3072}, f32);
    auto A1 = T_({2688, 3072}, bf), B1 = T_({2688, 768}, bf), C1 = T_({3072, 768}, f32), wsp = T_({8 * 2 * 2359296}, f32);
    expect_ok("dw2", [&] { gemm_dw2(A0, B0, C0, A1, B1, C1, wsp, false, {}, {}, false); });
  }
  // ---- split-K small-M GEMM + fused epilogues (splitk.hip)
  {
    auto A = T_({64, 3072}, bf), Bt = T_({768, 3072}, bf), C = T_({64, 768}, bf), ws = T_({256 * 64 * 64 + 64 * 768}, f32);
    auto res = T_({64, 768}, bf), g = T_({768}, f32), b = T_({768}, f32), mean = T_({64}, f32), rstd = T_({64}, f32);
    auto z = T_({64, 768}, bf), dx = T_({64, 768}, bf), cp = T_({64 * 3 * 768}, f32), sd = T_({1}, i32);
    const c10::optional<at::Tensor> o_b = b, o_res = res, o_g = g, o_m = mean, o_r = rstd, o_z = z, o_dx = dx, o_cp = cp,
                                    o_sd = sd;
    expect_ok("splitk bf16", [&] { gemm_splitk(0, A, Bt, C, ws, 0, none, none, none, none, none, none, none, none, none,
                                               none, none, none, 1e-12, none, 0, 0, 1.0, none); });
    expect_ok("splitk ln fwd", [&] { gemm_splitk(6, A, Bt, C, ws, 0, o_b, none, none, o_res, none, o_g, o_b, o_m, o_r,
                                                 o_z, none, none, 1e-12, o_sd, 9, 1000, 1.1, none); });
    expect_ok("splitk ln bwd", [&] { gemm_splitk(7, A, Bt, C, ws, 0, none, none, none, o_res, none, o_g, none, o_m, o_r,
                                                 o_z, o_dx, o_cp, 1e-12, o_sd, 9, 1000, 1.1, none); });
    expect_reject("splitk ln bwd colpart", [&] {
      gemm_splitk(7, A, Bt, C, ws, 0, none, none, none, o_res, none, o_g, none, o_m, o_r, o_z, o_dx,
                  c10::optional<at::Tensor>(T_({64 * 768}, f32)), 1e-12, o_sd, 9, 1000, 1.1, none); });
    expect_reject("splitk K mismatch", [&] { gemm_splitk(0, A, T_({768, 768}, bf), C, ws, 0, none, none, none, none,
                                                         none, none, none, none, none, none, none, none, 1e-12, none,
                                                         0, 0, 1.0, none); });
    expect_reject("splitk bias missing", [&] { gemm_splitk(1, A, Bt, C, ws, 0, none, none, none, none, none, none, none,
                                                           none, none, none, none, none, 1e-12, none, 0, 0, 1.0, none); });
  }
  // ---- attention (padded and varlen), S up to 512
  {
    const int64_t B = 4, S = 128, H = 12, rows = B * S;
    auto qkv = T_({rows, 3 * H * 64}, bf), kb = T_({B, S}, f32), ctx = T_({rows, H * 64}, bf);
    auto lse = T_({B, H, S}, f32), seed = T_({1}, i32), dctx = T_({rows, H * 64}, bf), delta = T_({B * H * S}, f32);
    auto dqkv = T_({rows, 3 * H * 64}, bf);
    expect_ok("attn fwd", [&] { attn_fwd(qkv, kb, ctx, lse, B, S, H, seed, 16, 429496730, 1.1, none, none); });
    expect_ok("attn bwd", [&] { attn_bwd(qkv, kb, ctx, lse, dctx, delta, dqkv, B, S, H, seed, 16, 0, 1.0, none, none); });
    auto cu = T_({B + 1}, i32), qv = T_({300, 3 * H * 64}, bf), cv = T_({300, H * 64}, bf);
    expect_ok("attn fwd varlen", [&] { attn_fwd(qv, kb, cv, lse, B, S, H, seed, 16, 0, 1.0, cu, none); });
    const int64_t S5 = 512;
    auto q5 = T_({2 * S5, 3 * H * 64}, bf), k5 = T_({2, S5}, f32), c5 = T_({2 * S5, H * 64}, bf), l5 = T_({2, H, S5}, f32);
    expect_ok("attn fwd S=512", [&] { attn_fwd(q5, k5, c5, l5, 2, S5, H, seed, 16, 0, 1.0, none, none); });
    expect_reject("attn S=576", [&] { attn_fwd(q5, k5, c5, l5, 2, 576, H, seed, 16, 0, 1.0, none, none); });
    expect_reject("attn S % 64", [&] { attn_fwd(qkv, kb, ctx, lse, B, 100, H, seed, 16, 0, 1.0, none, none); });
    expect_reject("attn lse size", [&] { attn_fwd(qkv, kb, ctx, l5, B, S, H, seed, 16, 0, 1.0, none, none); });
    auto cu_bad = T_({B}, i32);
    expect_reject("attn cu size", [&] { attn_fwd(qv, kb, cv, lse, B, S, H, seed, 16, 0, 1.0, cu_bad, none); });
    auto dm = T_({B * H * 256}, i64), dm_bad = T_({B * H * 100}, i64);
    expect_ok("attn fwd + keep bits", [&] { attn_fwd(qkv, kb, ctx, lse, B, S, H, seed, 16, 429496730, 1.1, none, dm); });
    expect_ok("attn bwd + keep bits", [&] { attn_bwd(qkv, kb, ctx, lse, dctx, delta, dqkv, B, S, H, seed, 16, 429496730,
                                                     1.1, none, dm); });
    expect_reject("attn dmask size", [&] { attn_fwd(qkv, kb, ctx, lse, B, S, H, seed, 16, 429496730, 1.1, none, dm_bad); });
    expect_reject("attn dmask S=512", [&] { attn_fwd(q5, k5, c5, l5, 2, S5, H, seed, 16, 0, 1.0, none, dm); });
    expect_reject("attn bwd dqkv size", [&] { attn_bwd(qkv, kb, ctx, lse, dctx, delta, ctx, B, S, H, seed, 16, 0, 1.0, none, none); });
    // fused QKV projection + attention (both modes): flags in the LayerNorm state's tail
    auto x = T_({rows, H * 64}, bf), w = T_({3 * H * 64, H * 64}, bf), bq = T_({3 * H * 64}, f32);
    auto stats = T_({4096}, i64), cnt = T_({2}, i32), err = T_({1}, i32);
    for (int64_t mode : {1, 2}) {
      expect_ok("qkv attn fwd", [&] { gemm_attn_fwd(x, w, bq, qkv, kb, ctx, lse, B, S, H, seed, 16, 429496730, 1.1,
                                                   none, dm, 0, stats, cnt, err, 2, none, none, none, none, mode); });
      auto xv = T_({300, H * 64}, bf);
      expect_ok("qkv attn fwd varlen", [&] { gemm_attn_fwd(xv, w, bq, qv, kb, cv, lse, B, S, H, seed, 16, 0, 1.0, cu,
                                                          none, 0, stats, cnt, err, 2, none, none, none, none, mode); });
    }
    expect_reject("qkv attn S=256", [&] { gemm_attn_fwd(x, w, bq, qkv, kb, ctx, lse, 2, 256, H, seed, 16, 0, 1.0, none,
                                                        none, 0, stats, cnt, err, 2, none, none, none, none, 1); });
    expect_reject("qkv attn w shape", [&] { gemm_attn_fwd(x, T_({2 * H * 64, H * 64}, bf), bq, qkv, kb, ctx, lse, B, S, H,
                                                          seed, 16, 0, 1.0, none, none, 0, stats, cnt, err, 2, none,
                                                          none, none, none, 1); });
    expect_reject("qkv attn stats", [&] { gemm_attn_fwd(x, w, bq, qkv, kb, ctx, lse, B, S, H, seed, 16, 0, 1.0, none,
                                                        none, 0, T_({1000}, i64), cnt, err, 2, none, none, none, none,
                                                        1); });
    expect_reject("qkv attn xsite", [&] { gemm_attn_fwd(x, w, bq, qkv, kb, ctx, lse, B, S, H, seed, 16, 0, 1.0, none,
                                                        none, 0, stats, cnt, err, 127, none, none, none, none, 1); });
    expect_ok("attn bwd proj", [&] { attn_bwd_proj(qkv, kb, ctx, lse, x, T_({H * 64, H * 64}, bf), dqkv, B, S, H, seed, 16,
                                                  429496730, 1.1, none, dm); });
    expect_ok("attn bwd proj varlen", [&] { attn_bwd_proj(qv, kb, cv, lse, T_({300, H * 64}, bf), T_({H * 64, H * 64}, bf),
                                                         T_({300, 3 * H * 64}, bf), B, S, H, seed, 16, 0, 1.0, cu, none); });
    expect_reject("attn bwd proj S=256", [&] { attn_bwd_proj(qkv, kb, ctx, lse, x, T_({H * 64, H * 64}, bf), dqkv, 2, 256,
                                                            H, seed, 16, 0, 1.0, none, none); });
    expect_reject("attn bwd proj w shape", [&] { attn_bwd_proj(qkv, kb, ctx, lse, x, T_({H * 64, 64}, bf), dqkv, B, S, H,
                                                              seed, 16, 0, 1.0, none, none); });
    expect_reject("qkv attn mode", [&] { gemm_attn_fwd(x, w, bq, qkv, kb, ctx, lse, B, S, H, seed, 16, 0, 1.0, none,
                                                       none, 0, stats, cnt, err, 2, none, none, none, none, 3); });
  }
  // ---- LayerNorm fwd / bwd
  {
    const int64_t Tn = 2688, D = 768;
    auto x = T_({Tn, D}, bf), r = T_({Tn, D}, bf), ga = T_({D}, f32), be = T_({D}, f32), y = T_({Tn, D}, bf);
    auto mean = T_({Tn}, f32), rstd = T_({Tn}, f32), seed = T_({1}, i32), rm = T_({Tn}, i32);
    expect_ok("ln fwd", [&] { ln_fwd(x, r, ga, be, y, mean, rstd, 1e-12, seed, 17, 429496730, 1.1, rm); });
    auto dz = T_({Tn, D}, bf), dx = T_({Tn, D}, bf), dg = T_({D}, f32), db = T_({D}, f32), dbias = T_({D}, f32);
    auto work = T_({336 * 3 * D}, f32);
    expect_ok("ln bwd", [&] { ln_bwd(x, x, r, ga, mean, rstd, dz, dx, dg, db, dbias, work, seed, 17, 429496730, 1.1,
                                     false, rm, true, false); });
    auto small = T_({100 * 3 * D}, f32);
    expect_reject("ln bwd work", [&] { ln_bwd(x, x, r, ga, mean, rstd, dz, dx, dg, db, dbias, small, seed, 17, 0, 1.0,
                                              false, none, false, false); });
    expect_reject("ln bwd dx with dropout", [&] { ln_bwd(x, x, r, ga, mean, rstd, dz, none, dg, db, dbias, work, seed,
                                                         17, 429496730, 1.1, false, none, false, false); });
    expect_ok("ln bwd from z", [&] { ln_bwd(x, x, none, ga, mean, rstd, dz, dx, dg, db, dbias, work, seed, 17, 429496730,
                                            1.1, false, rm, true, true); });
    expect_reject("ln bwd z + residual", [&] { ln_bwd(x, x, r, ga, mean, rstd, dz, dx, dg, db, dbias, work, seed, 17, 0,
                                                      1.0, false, none, false, true); });
    auto g2 = T_({1024}, f32);
    expect_reject("ln fwd D", [&] { ln_fwd(x, r, g2, g2, y, mean, rstd, 1e-12, seed, 17, 0, 1.0, none); });
    auto rm_bad = T_({10}, i32);
    expect_reject("ln fwd row_map", [&] { ln_fwd(x, r, ga, be, y, mean, rstd, 1e-12, seed, 17, 0, 1.0, rm_bad); });
    // LayerNorm fused into the N = 768 GEMM (forward: out_lin / lin2; backward: the dX GEMM)
    auto a = T_({Tn, 3072}, bf), wt = T_({D, 3072}, bf), bias = T_({D}, f32), z = T_({Tn, D}, bf);
    auto stats = T_({2 * (Tn + 128) * (D / 64)}, i64), cnt = T_({2}, i32), err = T_({1}, i32);
    auto cp = T_({((Tn + 63) / 64) * 3 * D}, f32);
    expect_ok("gemm_ln fwd", [&] { gemm_ln(false, a, wt, y, bias, r, ga, be, mean, rstd, z, none, none, stats, cnt, err,
                                           1e-12, seed, 17, 429496730, 1.1, rm, -1, 0); });
    expect_ok("gemm_ln bwd", [&] { gemm_ln(true, a, wt, dz, none, r, ga, none, mean, rstd, z, dx, cp, stats, cnt, err,
                                           1e-12, seed, 17, 429496730, 1.1, rm, -1, 0); });
    expect_reject("gemm_ln bwd without z", [&] { gemm_ln(true, a, wt, dz, none, r, ga, none, mean, rstd, none, dx, cp,
                                                         stats, cnt, err, 1e-12, seed, 17, 0, 1.0, none, -1, 0); });
    expect_reject("gemm_ln bwd dropout without dx", [&] {
      gemm_ln(true, a, wt, dz, none, r, ga, none, mean, rstd, z, none, cp, stats, cnt, err, 1e-12, seed, 17, 429496730,
              1.1, rm, -1, 0); });
    auto stats_small = T_({100}, i64);
    expect_reject("gemm_ln stats size", [&] { gemm_ln(false, a, wt, y, bias, r, ga, be, mean, rstd, z, none, none,
                                                      stats_small, cnt, err, 1e-12, seed, 17, 0, 1.0, none, -1, 0); });
    expect_reject("gemm_ln fwd without beta", [&] { gemm_ln(false, a, wt, y, bias, r, ga, none, mean, rstd, z, none,
                                                            none, stats, cnt, err, 1e-12, seed, 17, 0, 1.0, none, -1, 0); });
    expect_reject("gemm_ln xsite range", [&] { gemm_ln(false, a, wt, y, bias, r, ga, be, mean, rstd, z, none, none,
                                                       stats, cnt, err, 1e-12, seed, 17, 0, 1.0, none, -1, 128); });
    auto cp_small = T_({3 * D}, f32);
    expect_reject("gemm_ln colpart size", [&] { gemm_ln(true, a, wt, dz, none, r, ga, none, mean, rstd, z, dx, cp_small,
                                                        stats, cnt, err, 1e-12, seed, 17, 0, 1.0, none, -1, 0); });
  }
  // ---- head (+ fused distillation loss)
  {
    const int64_t B = 32, S = 128, D = 768;
    auto hid = T_({B * S, D}, bf), W = T_({2, D}, f32), bias = T_({2}, f32), seed = T_({1}, i32);
    auto lab = T_({B}, i64), logits = T_({B, 2}, f32), loss = T_({}, f32), dlog = T_({B, 2}, f32), rl = T_({B}, f32);
    auto tl = T_({B, 2}, f32);
    expect_ok("head fwd", [&] { head_fwd(hid, B, S, W, bias, seed, 2, 0, 1.0, lab, logits, loss, dlog, rl, none,
                                         none, 1.0, 1.0, none); });
    const c10::optional<at::Tensor> lacc = T_({1}, f32);
    expect_ok("head fwd loss_acc", [&] { head_fwd(hid, B, S, W, bias, seed, 2, 0, 1.0, lab, logits, loss, dlog, rl,
                                                  none, none, 1.0, 1.0, lacc); });
    expect_ok("head fwd kd", [&] { head_fwd(hid, B, S, W, bias, seed, 2, 0, 1.0, lab, logits, loss, dlog, rl, none, tl,
                                            2.0, 0.5, none); });
    expect_reject("head kd without labels", [&] { head_fwd(hid, B, S, W, bias, seed, 2, 0, 1.0, none, logits, none,
                                                           none, none, none, tl, 2.0, 0.5, none); });
    expect_reject("head kd T <= 0", [&] { head_fwd(hid, B, S, W, bias, seed, 2, 0, 1.0, lab, logits, loss, dlog, rl,
                                                   none, tl, 0.0, 0.5, none); });
    auto dW = T_({2, D}, f32), db = T_({2}, f32), dh = T_({B * S, D}, bf);
    expect_ok("head bwd", [&] { head_bwd(hid, B, S, W, seed, 2, 0, 1.0, dlog, dW, db, dh, false, none, none, none); });
    auto hid_small = T_({B * S - 1, D}, bf);
    expect_reject("head bwd hidden size", [&] { head_bwd(hid_small, B, S, W, seed, 2, 0, 1.0, dlog, dW, db, hid_small,
                                                         false, none, none, none); });
  }
  // ---- Adam over an arena with a run table (the fused-step remainder)
  {
    const int64_t n = 4096;
    auto p = T_({n}, f32), g = T_({n}, f32), m = T_({n}, f32), v = T_({n}, f32), sh = T_({n}, bf), step = T_({1}, i32);
    auto runs = T_({2, 3}, i64);
    auto rp = runs.data_ptr<int64_t>();
    rp[0] = 0; rp[1] = 64; rp[2] = 0; rp[3] = 512; rp[4] = 256; rp[5] = 64;
    expect_ok("adam runs", [&] { adam(p, g, m, v, sh, step, 2e-5, 0.9, 0.999, 1e-8, 0, false, none, none, 0, 0, 4,
                                      runs, 320, 768); });
    expect_reject("adam run end outside", [&] { adam(p, g, m, v, sh, step, 2e-5, 0.9, 0.999, 1e-8, 0, false, none,
                                                     none, 0, 0, 4, runs, 320, 4096); });
    auto g_small = T_({n - 4}, f32);
    expect_reject("adam sizes", [&] { adam(p, g_small, m, v, sh, step, 2e-5, 0.9, 0.999, 1e-8, 0, false, none, none,
                                           0, 0, 4, none, 0, 0); });
    // the sparse word-embedding rows (64 rows of 64)
    auto ever = T_({64}, at::kByte), now = T_({64}, at::kByte), ever_small = T_({10}, at::kByte);
    expect_ok("adam rows", [&] { adam_rows(p, g, m, v, sh, step, 2e-5, 0.9, 0.999, 1e-8, ever, now, 64); });
    expect_reject("adam rows flags", [&] { adam_rows(p, g, m, v, sh, step, 2e-5, 0.9, 0.999, 1e-8, ever_small, now,
                                                     64); });
    expect_reject("adam rows row_len", [&] { adam_rows(p, g, m, v, sh, step, 2e-5, 0.9, 0.999, 1e-8, ever, now, 6); });
    // parameter groups: a weight decay per run
    const c10::optional<at::Tensor> rwd = T_({2}, f32), rwd3 = T_({3}, f32);
    expect_ok("adam run decays", [&] { adam(p, g, m, v, sh, step, 2e-5, 0.9, 0.999, 1e-8, 0.01, true, none, none, 0, 0,
                                            4, runs, 320, 768, rwd, {0.01, 0.0}); });
    expect_reject("adam run decays length", [&] { adam(p, g, m, v, sh, step, 2e-5, 0.9, 0.999, 1e-8, 0.01, true, none,
                                                       none, 0, 0, 4, runs, 320, 768, rwd3, {0.01, 0.0, 0.0}); });
    expect_reject("adam run decays host length", [&] { adam(p, g, m, v, sh, step, 2e-5, 0.9, 0.999, 1e-8, 0.01, true,
                                                            none, none, 0, 0, 4, runs, 320, 768, rwd, {0.01}); });
    expect_reject("adam run decay negative", [&] { adam(p, g, m, v, sh, step, 2e-5, 0.9, 0.999, 1e-8, 0.01, true, none,
                                                        none, 0, 0, 4, runs, 320, 768, rwd, {0.01, -0.01}); });
    expect_reject("adam run decay NaN", [&] { adam(p, g, m, v, sh, step, 2e-5, 0.9, 0.999, 1e-8, 0.01, true, none, none,
                                                   0, 0, 4, runs, 320, 768, rwd, {0.01, std::nan("")}); });
    expect_reject("adam run decays without runs", [&] { adam(p, g, m, v, sh, step, 2e-5, 0.9, 0.999, 1e-8, 0.01, true,
                                                             none, none, 0, 0, 4, none, 0, 0, rwd, {0.01, 0.0}); });
    expect_reject("adam weight decay negative", [&] { adam(p, g, m, v, sh, step, 2e-5, 0.9, 0.999, 1e-8, -0.01, true,
                                                           none, none, 0, 0, 4, none, 0, 0); });
    // flagged rows under weight decay: decoupled only (the other rows decay lazily)
    expect_ok("adam rows decoupled decay", [&] { adam_rows(p, g, m, v, sh, step, 2e-5, 0.9, 0.999, 1e-8, ever, now, 64,
                                                           0.01, true); });
    expect_reject("adam rows coupled decay", [&] { adam_rows(p, g, m, v, sh, step, 2e-5, 0.9, 0.999, 1e-8, ever, now,
                                                             64, 0.01, false); });
    expect_ok("adam flags decoupled decay", [&] { adam(p, g, m, v, sh, step, 2e-5, 0.9, 0.999, 1e-8, 0.01, true, ever,
                                                       now, 0, 64, 64, none, 0, 0); });
    expect_reject("adam flags coupled decay", [&] { adam(p, g, m, v, sh, step, 2e-5, 0.9, 0.999, 1e-8, 0.01, false, ever,
                                                         now, 0, 64, 64, none, 0, 0); });
    // the lazy decay of rows without state (all rows, or the rows of a batch's ids)
    auto done = T_({64}, i32), done_small = T_({10}, i32), ids = T_({4, 8}, i64), ids32 = T_({32}, i32);
    expect_ok("lazy decay all rows", [&] { adam_lazy_decay(p, sh, done, ever, step, 0, 2e-5, 0.01, 64, none); });
    expect_ok("lazy decay ids", [&] { adam_lazy_decay(p, sh, done, ever, step, 1, 2e-5, 0.01, 64, ids); });
    expect_ok("lazy decay int32 ids", [&] { adam_lazy_decay(p, none, done, ever, step, 0, 2e-5, 0.01, 64, ids32); });
    expect_reject("lazy decay counters", [&] { adam_lazy_decay(p, sh, done_small, ever, step, 0, 2e-5, 0.01, 64, none); });
    expect_reject("lazy decay flags", [&] { adam_lazy_decay(p, sh, done, ever_small, step, 0, 2e-5, 0.01, 64, none); });
    expect_reject("lazy decay row_len", [&] { adam_lazy_decay(p, sh, done, ever, step, 0, 2e-5, 0.01, 6, none); });
    expect_reject("lazy decay adj", [&] { adam_lazy_decay(p, sh, done, ever, step, 2, 2e-5, 0.01, 64, none); });
    expect_reject("lazy decay negative", [&] { adam_lazy_decay(p, sh, done, ever, step, 0, 2e-5, -0.01, 64, none); });
    expect_reject("lazy decay ids dtype", [&] { adam_lazy_decay(p, sh, done, ever, step, 0, 2e-5, 0.01, 64, g); });
    // learning-rate schedules [kind, warmup, total, offset] on every Adam entry point
    const std::vector<int64_t> lin = {1, 3, 10, 0}, cww = {2, 3, 0, 7}, edge = {1, 5, 5, 0}, cst = {0, 0, 0, 0};
    const std::vector<std::vector<int64_t>> bad = {{3, 0, 10, 0},  {-1, 0, 10, 0}, {1, -1, 10, 0}, {1, 2, -10, 0},
                                                   {1, 2, 10, -1}, {1, 11, 10, 0}, {1, 3, 10},     {1, 0, int64_t(1) << 31, 0}};
    for (const auto& sc : {lin, cww, edge, cst}) {
      expect_ok("adam sched", [&] { adam(p, g, m, v, sh, step, 2e-5, 0.9, 0.999, 1e-8, 0.01, true, none, none, 0, 0, 4,
                                         runs, 320, 768, rwd, {0.01, 0.0}, sc); });
      expect_ok("adam rows sched", [&] { adam_rows(p, g, m, v, sh, step, 2e-5, 0.9, 0.999, 1e-8, ever, now, 64, 0.01,
                                                   true, sc); });
      expect_ok("lazy decay sched", [&] { adam_lazy_decay(p, sh, done, ever, step, 1, 2e-5, 0.01, 64, ids, sc); });
      auto tab = T_({12}, f32);
      expect_ok("lr table", [&] { lr_schedule_table(tab, 2e-5, sc); });
    }
    for (const auto& sc : bad) {
      expect_reject("adam sched bad", [&] { adam(p, g, m, v, sh, step, 2e-5, 0.9, 0.999, 1e-8, 0, false, none, none, 0, 0,
                                                 4, runs, 320, 768, none, {}, sc); });
      expect_reject("adam rows sched bad", [&] { adam_rows(p, g, m, v, sh, step, 2e-5, 0.9, 0.999, 1e-8, ever, now, 64,
                                                           0.0, false, sc); });
      expect_reject("lazy decay sched bad", [&] { adam_lazy_decay(p, sh, done, ever, step, 0, 2e-5, 0.01, 64, none, sc); });
      auto tab = T_({12}, f32);
      expect_reject("lr table sched bad", [&] { lr_schedule_table(tab, 2e-5, sc); });
    }
    // (warmup > total is fine for the constant-with-warmup kind, whose total is unused)
    expect_ok("adam rows sched warmup only", [&] { adam_rows(p, g, m, v, sh, step, 2e-5, 0.9, 0.999, 1e-8, ever, now, 64,
                                                             0.0, false, {2, 11, 10, 0}); });
    expect_reject("adam lr inf", [&] { adam(p, g, m, v, sh, step, INFINITY, 0.9, 0.999, 1e-8, 0, false, none, none, 0, 0,
                                            4, runs, 320, 768, none, {}, lin); });
    expect_reject("adam rows lr NaN", [&] { adam_rows(p, g, m, v, sh, step, std::nan(""), 0.9, 0.999, 1e-8, ever, now,
                                                      64); });
    // FedProx: the anchor is laid out like p
    {
      const c10::optional<at::Tensor> anc = T_({n}, f32), anc_short = T_({n - 4}, f32), anc_bf = T_({n}, bf);
      expect_ok("adam prox", [&] { adam(p, g, m, v, sh, step, 2e-5, 0.9, 0.999, 1e-8, 0.01, true, none, none, 0, 0, 4,
                                        runs, 320, 768, none, {}, {}, 0.1, anc); });
      expect_ok("adam prox mu 0, no anchor", [&] { adam(p, g, m, v, sh, step, 2e-5, 0.9, 0.999, 1e-8, 0, false, none,
                                                        none, 0, 0, 4, runs, 320, 768, none, {}, {}, 0.0, none); });
      expect_ok("adam prox flags", [&] { adam(p, g, m, v, sh, step, 2e-5, 0.9, 0.999, 1e-8, 0, false, ever, now, 0, 64,
                                              64, none, 0, 0, none, {}, {}, 0.1, anc); });
      expect_reject("adam prox no anchor", [&] { adam(p, g, m, v, sh, step, 2e-5, 0.9, 0.999, 1e-8, 0, false, none, none,
                                                      0, 0, 4, runs, 320, 768, none, {}, {}, 0.1, none); });
      expect_reject("adam prox short anchor", [&] { adam(p, g, m, v, sh, step, 2e-5, 0.9, 0.999, 1e-8, 0, false, none,
                                                         none, 0, 0, 4, runs, 320, 768, none, {}, {}, 0.1, anc_short); });
      expect_reject("adam prox short anchor, mu 0", [&] { adam(p, g, m, v, sh, step, 2e-5, 0.9, 0.999, 1e-8, 0, false,
                                                               none, none, 0, 0, 4, runs, 320, 768, none, {}, {}, 0.0,
                                                               anc_short); });
      expect_reject("adam prox anchor dtype", [&] { adam(p, g, m, v, sh, step, 2e-5, 0.9, 0.999, 1e-8, 0, false, none,
                                                         none, 0, 0, 4, runs, 320, 768, none, {}, {}, 0.1, anc_bf); });
      expect_reject("adam prox mu negative", [&] { adam(p, g, m, v, sh, step, 2e-5, 0.9, 0.999, 1e-8, 0, false, none,
                                                        none, 0, 0, 4, runs, 320, 768, none, {}, {}, -0.1, anc); });
      expect_reject("adam prox mu NaN", [&] { adam(p, g, m, v, sh, step, 2e-5, 0.9, 0.999, 1e-8, 0, false, none, none, 0,
                                                   0, 4, runs, 320, 768, none, {}, {}, std::nan(""), anc); });
      expect_reject("adam prox flags + decay", [&] { adam(p, g, m, v, sh, step, 2e-5, 0.9, 0.999, 1e-8, 0.01, true, ever,
                                                          now, 0, 64, 64, none, 0, 0, none, {}, {}, 0.1, anc); });
      expect_ok("adam rows prox", [&] { adam_rows(p, g, m, v, sh, step, 2e-5, 0.9, 0.999, 1e-8, ever, now, 64, 0.0, false,
                                                  {}, 0.1, anc); });
      expect_reject("adam rows prox no anchor", [&] { adam_rows(p, g, m, v, sh, step, 2e-5, 0.9, 0.999, 1e-8, ever, now,
                                                                64, 0.0, false, {}, 0.1, none); });
      expect_reject("adam rows prox short anchor", [&] { adam_rows(p, g, m, v, sh, step, 2e-5, 0.9, 0.999, 1e-8, ever,
                                                                   now, 64, 0.0, false, {}, 0.1, anc_short); });
      expect_reject("adam rows prox + decay", [&] { adam_rows(p, g, m, v, sh, step, 2e-5, 0.9, 0.999, 1e-8, ever, now, 64,
                                                              0.01, true, {}, 0.1, anc); });
    }
    expect_reject("lr table lr NaN", [&] { lr_schedule_table(T_({4}, f32), std::nan(""), lin); });
    expect_reject("lr table empty", [&] { lr_schedule_table(T_({0}, f32), 2e-5, lin); });
    expect_reject("lr table no schedule", [&] { lr_schedule_table(T_({4}, f32), 2e-5, {}); });
  }
  // ---- invalid hyper-parameters: ONE table against every entry that builds an FdAdamHyper (adam,
  // adam_rows, adam_lazy_decay, gemm_dw_batch with and without the rest of the step).  Each entry
  // first accepts the table's base values with the very tensors the rows use, so a rejection is the
  // row's doing; each row must then be refused before any launcher call.  (adam_lazy_decay takes
  // no proximal term: the mu rows do not apply to it.)
  {
    const int64_t n = 4096, an = 64 * 64 + 1024;
    auto p = T_({n}, f32), g = T_({n}, f32), m = T_({n}, f32), v = T_({n}, f32), sh = T_({n}, bf), step = T_({1}, i32);
    auto ever = T_({64}, at::kByte), now = T_({64}, at::kByte), done = T_({64}, i32);
    const c10::optional<at::Tensor> anc = T_({n}, f32);
    std::vector<at::Tensor> As = {T_({64, 128}, bf)}, Bs = {T_({64, 64}, bf)}, Cs = {T_({128, 64}, f32)};
    std::vector<at::Tensor> st = {T_({128 * 64}, f32), T_({128 * 64}, f32), T_({128 * 64}, f32), T_({128 * 64}, bf), step};
    std::vector<at::Tensor> rest = {T_({an}, f32), T_({an}, f32), T_({an}, f32), T_({an}, f32), T_({an}, bf),
                                    T_({2, 3}, i64), T_({64}, at::kByte), T_({64}, at::kByte)};
    auto rp = rest[5].data_ptr<int64_t>();
    rp[0] = 1024; rp[1] = 128; rp[2] = 0; rp[3] = 1152; rp[4] = 128; rp[5] = 128;
    const std::vector<int64_t> ri = {256, 0, 64, 64}, acc = {0};
    const std::vector<at::Tensor> danc = {T_({128 * 64}, f32)}, danc_rest = {danc[0], T_({an}, f32)};
    struct Hyper { const char* name; double lr, wd, mu; std::vector<int64_t> sched; };
    const double inf = HUGE_VAL, nan = std::nan("");
    const int64_t lim = int64_t(1) << 30;
    const Hyper base = {"base", 2e-5, 0.0, 0.05, {1, 3, 10, 0}};
    const std::vector<Hyper> bad = {
        {"mu negative", 2e-5, 0.0, -0.1, {}},          {"mu NaN", 2e-5, 0.0, nan, {}},
        {"mu inf", 2e-5, 0.0, inf, {}},                {"wd negative", 2e-5, -0.01, 0.05, {}},
        {"wd NaN", 2e-5, nan, 0.05, {}},               {"wd inf", 2e-5, inf, 0.05, {}},
        {"lr inf", inf, 0.0, 0.05, {}},                {"lr -inf", -inf, 0.0, 0.05, {}},
        {"lr NaN", nan, 0.0, 0.05, {}},                {"sched kind 3", 2e-5, 0.0, 0.05, {3, 0, 10, 0}},
        {"sched kind -1", 2e-5, 0.0, 0.05, {-1, 0, 10, 0}}, {"sched warmup -1", 2e-5, 0.0, 0.05, {1, -1, 10, 0}},
        {"sched total -10", 2e-5, 0.0, 0.05, {1, 2, -10, 0}}, {"sched offset -1", 2e-5, 0.0, 0.05, {1, 2, 10, -1}},
        {"sched warmup > total", 2e-5, 0.0, 0.05, {1, 11, 10, 0}}, {"sched 3 entries", 2e-5, 0.0, 0.05, {1, 3, 10}},
        {"sched total 2^31", 2e-5, 0.0, 0.05, {1, 0, int64_t(1) << 31, 0}},
        {"sched total 2^30", 2e-5, 0.0, 0.05, {1, 0, lim, 0}}, {"sched warmup 2^30", 2e-5, 0.0, 0.05, {2, lim, 0, 0}},
        {"sched offset 2^30", 2e-5, 0.0, 0.05, {1, 0, 10, lim}}};
    // (decoupled decay throughout, so the base and the wd rows differ in nothing but the value)
    auto e_adam = [&](const Hyper& h) { adam(p, g, m, v, sh, step, h.lr, 0.9, 0.999, 1e-8, h.wd, true, none, none, 0, 0,
                                             4, none, 0, 0, none, {}, h.sched, h.mu, anc); };
    auto e_rows = [&](const Hyper& h) { adam_rows(p, g, m, v, sh, step, h.lr, 0.9, 0.999, 1e-8, ever, now, 64, h.wd,
                                                  true, h.sched, h.mu, anc); };
    auto e_lazy = [&](const Hyper& h) { adam_lazy_decay(p, sh, done, ever, step, 0, h.lr, h.wd, 64, none, h.sched); };
    auto e_dwb = [&](const Hyper& h) { gemm_dw_batch(As, Bs, Cs, acc, st, {h.lr, 0.9, 0.999, 1e-8, h.wd, 1.0}, -1, {},
                                                     {}, {}, {}, {}, none, {}, 0.0, h.sched, h.mu, danc); };
    auto e_dwb_rest = [&](const Hyper& h) { gemm_dw_batch(As, Bs, Cs, acc, st, {h.lr, 0.9, 0.999, 1e-8, h.wd, 1.0}, -1,
                                                          {}, rest, ri, {}, {}, none, {}, 0.0, h.sched, h.mu,
                                                          danc_rest); };
    expect_ok("hyper table base: adam", [&] { e_adam(base); });
    expect_ok("hyper table base: adam_rows", [&] { e_rows(base); });
    expect_ok("hyper table base: adam_lazy_decay", [&] { e_lazy(base); });
    expect_ok("hyper table base: dw_batch", [&] { e_dwb(base); });
    expect_ok("hyper table base: dw_batch rest", [&] { e_dwb_rest(base); });
    for (const Hyper& h : bad) {
      const std::string nm = std::string("hyper table, ") + h.name + ": ";
      expect_reject((nm + "adam").c_str(), [&] { e_adam(h); });
      expect_reject((nm + "adam_rows").c_str(), [&] { e_rows(h); });
      if (h.mu == base.mu) expect_reject((nm + "adam_lazy_decay").c_str(), [&] { e_lazy(h); });
      expect_reject((nm + "dw_batch").c_str(), [&] { e_dwb(h); });
      expect_reject((nm + "dw_batch rest").c_str(), [&] { e_dwb_rest(h); });
    }
  }
  // ---- FedOpt server step: four fp32 streams, the bf16 shadow, two stats floats per block
  {
    const int64_t n = 4096 * 1024 + 4 * 257;  // the grid-stride loop wraps, ragged last block
    const int64_t nb = 2 * fd_server_opt_grid(n);
    auto ms = T_({n}, f32), x = T_({n}, f32), m = T_({n}, f32), v = T_({n}, f32), sh = T_({n}, bf), st = T_({nb}, f32);
    expect_ok("server_opt avgm", [&] { server_opt(ms, x, m, none, sh, 0, 0.5, 1.0, 0.9, 0.99, 1e-3, st); });
    expect_ok("server_opt adagrad", [&] { server_opt(ms, x, m, v, sh, 1, 0.5, 1e-2, 0.9, 0.99, 1e-3, st); });
    expect_ok("server_opt adam", [&] { server_opt(ms, x, m, v, sh, 2, 0.5, 1e-2, 0.9, 0.99, 1e-3, st); });
    expect_ok("server_opt yogi, no shadow / stats", [&] { server_opt(ms, x, m, v, none, 3, 0.5, 1e-2, 0.9, 0.99, 1e-3,
                                                                     none); });
    auto s8 = T_({2048}, f32), x8 = T_({2048}, f32), m8 = T_({2048}, f32), st8 = T_({2 * 2}, f32);
    expect_ok("server_opt small", [&] { server_opt(s8, x8, m8, none, none, 0, 0.5, 1.0, 0.0, 0.0, 1e-3, st8); });
    auto xs = T_({n - 4}, f32), msh = T_({n - 4}, f32), vs = T_({n - 4}, f32), shs = T_({n - 4}, bf);
    expect_reject("server_opt short x", [&] { server_opt(ms, xs, m, v, sh, 2, 0.5, 1e-2, 0.9, 0.99, 1e-3, st); });
    expect_reject("server_opt short m", [&] { server_opt(ms, x, msh, v, sh, 2, 0.5, 1e-2, 0.9, 0.99, 1e-3, st); });
    expect_reject("server_opt short v", [&] { server_opt(ms, x, m, vs, sh, 2, 0.5, 1e-2, 0.9, 0.99, 1e-3, st); });
    expect_reject("server_opt short shadow", [&] { server_opt(ms, x, m, v, shs, 2, 0.5, 1e-2, 0.9, 0.99, 1e-3, st); });
    expect_reject("server_opt adam without v", [&] { server_opt(ms, x, m, none, sh, 2, 0.5, 1e-2, 0.9, 0.99, 1e-3,
                                                                st); });
    expect_reject("server_opt avgm with v", [&] { server_opt(ms, x, m, v, sh, 0, 0.5, 1.0, 0.9, 0.99, 1e-3, st); });
    expect_reject("server_opt kind", [&] { server_opt(ms, x, m, v, sh, 4, 0.5, 1e-2, 0.9, 0.99, 1e-3, st); });
    auto xb = T_({n}, bf), shf = T_({n}, f32), sti = T_({nb}, i32);
    expect_reject("server_opt x dtype", [&] { server_opt(ms, xb, m, v, sh, 2, 0.5, 1e-2, 0.9, 0.99, 1e-3, st); });
    expect_reject("server_opt shadow dtype", [&] { server_opt(ms, x, m, v, shf, 2, 0.5, 1e-2, 0.9, 0.99, 1e-3, st); });
    expect_reject("server_opt stats dtype", [&] { server_opt(ms, x, m, v, sh, 2, 0.5, 1e-2, 0.9, 0.99, 1e-3, sti); });
    auto st_short = T_({nb - 1}, f32);
    expect_reject("server_opt short stats", [&] { server_opt(ms, x, m, v, sh, 2, 0.5, 1e-2, 0.9, 0.99, 1e-3,
                                                             st_short); });
    auto s6 = T_({2046}, f32), x6 = T_({2046}, f32), m6 = T_({2046}, f32);
    expect_reject("server_opt numel % 4", [&] { server_opt(s6, x6, m6, none, none, 0, 0.5, 1.0, 0.9, 0.99, 1e-3,
                                                           none); });
    auto xt = T_({2, n / 2}, f32).t();
    expect_reject("server_opt non-contiguous x", [&] { server_opt(ms, xt, m, v, sh, 2, 0.5, 1e-2, 0.9, 0.99, 1e-3,
                                                                  st); });
    const double inf = HUGE_VAL;
    expect_reject("server_opt eta NaN", [&] { server_opt(ms, x, m, v, sh, 2, 0.5, std::nan(""), 0.9, 0.99, 1e-3, st); });
    expect_reject("server_opt eta inf", [&] { server_opt(ms, x, m, v, sh, 2, 0.5, inf, 0.9, 0.99, 1e-3, st); });
    expect_reject("server_opt eta 0", [&] { server_opt(ms, x, m, v, sh, 2, 0.5, 0.0, 0.9, 0.99, 1e-3, st); });
    expect_reject("server_opt tau 0", [&] { server_opt(ms, x, m, v, sh, 2, 0.5, 1e-2, 0.9, 0.99, 0.0, st); });
    expect_reject("server_opt b1 = 1", [&] { server_opt(ms, x, m, v, sh, 2, 0.5, 1e-2, 1.0, 0.99, 1e-3, st); });
    expect_reject("server_opt b2 < 0", [&] { server_opt(ms, x, m, v, sh, 2, 0.5, 1e-2, 0.9, -0.1, 1e-3, st); });
    expect_reject("server_opt inv inf", [&] { server_opt(ms, x, m, v, sh, 2, inf, 1e-2, 0.9, 0.99, 1e-3, st); });
  }
  // ---- robust aggregation: M fp32 sources, out, the bf16 shadow, 17 count ints per block
  {
    const int64_t n = 4096 * 1024 + 4 * 257;  // the grid-stride loop wraps, ragged last block
    const int64_t nc = 17 * fd_robust_agg_grid(n);
    std::vector<at::Tensor> s3, s16, s17;
    for (int i = 0; i < 17; ++i) {
      auto t = T_({n}, f32);
      if (i < 3) s3.push_back(t);
      if (i < 16) s16.push_back(t);
      s17.push_back(t);
    }
    auto out = T_({n}, f32), sh = T_({n}, bf), ct = T_({nc}, i32);
    expect_ok("robust_agg M 3 median", [&] { robust_agg(s3, 1, out, sh, ct); });
    expect_ok("robust_agg M 3 mean, no shadow / counts", [&] { robust_agg(s3, 0, out, none, none); });
    expect_ok("robust_agg M 16 median", [&] { robust_agg(s16, 7, out, sh, ct); });
    expect_ok("robust_agg M 2", [&] { robust_agg({s3[0], s3[1]}, 0, out, sh, none); });
    std::vector<at::Tensor> sm;
    for (int i = 0; i < 5; ++i) sm.push_back(T_({2048}, f32));
    auto o8 = T_({2048}, f32), c8 = T_({17 * 2}, i32);
    expect_ok("robust_agg small", [&] { robust_agg(sm, 2, o8, none, c8); });
    expect_reject("robust_agg M 1", [&] { robust_agg({s3[0]}, 0, out, sh, ct); });
    expect_reject("robust_agg M 17", [&] { robust_agg(s17, 1, out, sh, ct); });
    expect_reject("robust_agg 2k = M", [&] { robust_agg(s16, 8, out, sh, ct); });
    expect_reject("robust_agg 2k > M", [&] { robust_agg(s3, 2, out, sh, ct); });
    expect_reject("robust_agg k < 0", [&] { robust_agg(s3, -1, out, sh, ct); });
    auto srt = T_({n - 4}, f32), shs = T_({n - 4}, bf), ct_short = T_({nc - 1}, i32);
    expect_reject("robust_agg short source", [&] { robust_agg({s3[0], srt, s3[2]}, 1, out, sh, ct); });
    expect_reject("robust_agg short out", [&] { robust_agg(s3, 1, srt, none, ct); });
    expect_reject("robust_agg short shadow", [&] { robust_agg(s3, 1, out, shs, ct); });
    expect_reject("robust_agg short counts", [&] { robust_agg(s3, 1, out, sh, ct_short); });
    auto sb = T_({n}, bf), shf = T_({n}, f32), ctf = T_({nc}, f32), ob = T_({n}, bf);
    expect_reject("robust_agg source dtype", [&] { robust_agg({s3[0], sb, s3[2]}, 1, out, sh, ct); });
    expect_reject("robust_agg out dtype", [&] { robust_agg(s3, 1, ob, sh, ct); });
    expect_reject("robust_agg shadow dtype", [&] { robust_agg(s3, 1, out, shf, ct); });
    expect_reject("robust_agg counts dtype", [&] { robust_agg(s3, 1, out, sh, ctf); });
    auto xt = T_({2, n / 2}, f32).t();
    expect_reject("robust_agg non-contiguous source", [&] { robust_agg({s3[0], s3[1], xt}, 1, out, sh, ct); });
    std::vector<at::Tensor> s6;
    for (int i = 0; i < 3; ++i) s6.push_back(T_({2046}, f32));
    auto o6 = T_({2046}, f32);
    expect_reject("robust_agg numel % 4", [&] { robust_agg(s6, 1, o6, none, none); });
    expect_reject("robust_agg out is a source", [&] { robust_agg(s3, 1, s3[1], sh, ct); });
    // out / shadow as a window of a source's allocation
    auto big = T_({2 * n}, f32);
    auto lo = big.narrow(0, 0, n), mid = big.narrow(0, n / 2, n), hi = big.narrow(0, n, n);
    expect_reject("robust_agg out overlaps a source", [&] { robust_agg({s3[0], lo, s3[2]}, 1, mid, sh, ct); });
    expect_ok("robust_agg out beside a source", [&] { robust_agg({s3[0], lo, s3[2]}, 1, hi, sh, ct); });
    auto shv = big.narrow(0, n / 2, n / 2).view(bf);
    expect_reject("robust_agg shadow overlaps a source", [&] { robust_agg({s3[0], lo, s3[2]}, 1, out, shv, ct); });
  }
  // ---- distance-based robust aggregation: M fp32 sources, fp64 partials, 20 ctl floats, fp64 stats
  {
    const auto f64 = at::kDouble;
    const int64_t n = 4096 * 1024 + 4 * 257;  // the grid-stride loop wraps, ragged last block
    const int64_t grid = fd_robust_dist_grid(n);
    std::vector<at::Tensor> s3, s16, s17;
    for (int i = 0; i < 17; ++i) {
      auto t = T_({n}, f32);
      if (i < 3) s3.push_back(t);
      if (i < 16) s16.push_back(t);
      s17.push_back(t);
    }
    auto p3 = T_({3 * grid}, f64), p16 = T_({120 * grid}, f64), w3 = T_({4 * grid}, f64), w16 = T_({17 * grid}, f64);
    auto ctl = T_({20}, f32), ks = T_({288}, f64), gs = T_({7 * 34}, f64);
    auto out = T_({n}, f32), sh = T_({n}, bf);
    expect_ok("robust_pairdist M 3", [&] { robust_pairdist(s3, p3); });
    expect_ok("robust_pairdist M 16", [&] { robust_pairdist(s16, p16); });
    expect_ok("robust_pairdist M 2", [&] { robust_pairdist({s3[0], s3[1]}, p3); });
    expect_reject("robust_pairdist M 1", [&] { robust_pairdist({s3[0]}, p3); });
    expect_reject("robust_pairdist M 17", [&] { robust_pairdist(s17, p16); });
    expect_reject("robust_pairdist short partial", [&] { robust_pairdist(s16, T_({120 * grid - 1}, f64)); });
    expect_reject("robust_pairdist partial dtype", [&] { robust_pairdist(s3, T_({3 * grid}, f32)); });
    auto srt = T_({n - 4}, f32), sb = T_({n}, bf);
    expect_reject("robust_pairdist short source", [&] { robust_pairdist({s3[0], srt, s3[2]}, p3); });
    expect_reject("robust_pairdist source dtype", [&] { robust_pairdist({s3[0], sb, s3[2]}, p3); });
    auto xt = T_({2, n / 2}, f32).t();
    expect_reject("robust_pairdist non-contiguous source", [&] { robust_pairdist({s3[0], s3[1], xt}, p3); });
    std::vector<at::Tensor> s6;
    for (int i = 0; i < 3; ++i) s6.push_back(T_({2046}, f32));
    expect_reject("robust_pairdist numel % 4", [&] { robust_pairdist(s6, p3); });

    expect_ok("robust_krum_finalize M 3", [&] { robust_krum_finalize(p3, grid, 3, 0, 3, ctl, ks); });
    expect_ok("robust_krum_finalize M 16", [&] { robust_krum_finalize(p16, grid, 16, 6, 10, ctl, ks); });
    expect_ok("robust_krum_finalize large f", [&] { robust_krum_finalize(p3, grid, 3, 40, 1, ctl, ks); });
    expect_reject("robust_krum_finalize M 1", [&] { robust_krum_finalize(p3, grid, 1, 0, 1, ctl, ks); });
    expect_reject("robust_krum_finalize M 17", [&] { robust_krum_finalize(p16, grid, 17, 0, 1, ctl, ks); });
    expect_reject("robust_krum_finalize f < 0", [&] { robust_krum_finalize(p3, grid, 3, -1, 1, ctl, ks); });
    expect_reject("robust_krum_finalize m 0", [&] { robust_krum_finalize(p3, grid, 3, 0, 0, ctl, ks); });
    expect_reject("robust_krum_finalize m > M", [&] { robust_krum_finalize(p3, grid, 3, 0, 4, ctl, ks); });
    expect_reject("robust_krum_finalize grid 0", [&] { robust_krum_finalize(p3, 0, 3, 0, 1, ctl, ks); });
    expect_reject("robust_krum_finalize grid past partial", [&] { robust_krum_finalize(p3, grid + 1, 3, 0, 1, ctl, ks); });
    expect_reject("robust_krum_finalize M past partial", [&] { robust_krum_finalize(p3, grid, 4, 0, 1, ctl, ks); });
    expect_reject("robust_krum_finalize short ctl", [&] { robust_krum_finalize(p3, grid, 3, 0, 1, T_({19}, f32), ks); });
    expect_reject("robust_krum_finalize short stats", [&] { robust_krum_finalize(p3, grid, 3, 0, 1, ctl, T_({287}, f64)); });
    expect_reject("robust_krum_finalize ctl dtype", [&] { robust_krum_finalize(p3, grid, 3, 0, 1, T_({20}, f64), ks); });
    expect_reject("robust_krum_finalize stats dtype", [&] { robust_krum_finalize(p3, grid, 3, 0, 1, ctl, T_({288}, f32)); });

    expect_ok("robust_wmean M 3", [&] { robust_wmean(s3, ctl, out, sh, w3); });
    expect_ok("robust_wmean M 16", [&] { robust_wmean(s16, ctl, out, sh, w16); });
    expect_ok("robust_wmean distances only", [&] { robust_wmean(s3, ctl, none, none, w3); });
    expect_ok("robust_wmean out only", [&] { robust_wmean(s3, ctl, out, none, none); });
    expect_reject("robust_wmean M 1", [&] { robust_wmean({s3[0]}, ctl, out, sh, w3); });
    expect_reject("robust_wmean M 17", [&] { robust_wmean(s17, ctl, out, sh, w16); });
    expect_reject("robust_wmean shadow without out", [&] { robust_wmean(s3, ctl, none, sh, w3); });
    expect_reject("robust_wmean short ctl", [&] { robust_wmean(s3, T_({16}, f32), out, sh, w3); });
    expect_reject("robust_wmean short out", [&] { robust_wmean(s3, ctl, srt, none, w3); });
    expect_reject("robust_wmean short shadow", [&] { robust_wmean(s3, ctl, out, T_({n - 4}, bf), w3); });
    expect_reject("robust_wmean short partial", [&] { robust_wmean(s3, ctl, out, sh, T_({4 * grid - 1}, f64)); });
    expect_reject("robust_wmean short source", [&] { robust_wmean({s3[0], srt, s3[2]}, ctl, out, sh, w3); });
    expect_reject("robust_wmean out dtype", [&] { robust_wmean(s3, ctl, sb, sh, w3); });
    expect_reject("robust_wmean shadow dtype", [&] { robust_wmean(s3, ctl, out, T_({n}, f32), w3); });
    expect_reject("robust_wmean partial dtype", [&] { robust_wmean(s3, ctl, out, sh, T_({4 * grid}, f32)); });
    expect_reject("robust_wmean ctl dtype", [&] { robust_wmean(s3, T_({20}, f64), out, sh, w3); });
    expect_reject("robust_wmean non-contiguous source", [&] { robust_wmean({s3[0], s3[1], xt}, ctl, out, sh, w3); });
    expect_reject("robust_wmean numel % 4", [&] { robust_wmean(s6, ctl, T_({2046}, f32), none, none); });
    expect_reject("robust_wmean out is a source", [&] { robust_wmean(s3, ctl, s3[1], sh, w3); });
    auto big = T_({2 * n}, f32);
    auto lo = big.narrow(0, 0, n), mid = big.narrow(0, n / 2, n), hi = big.narrow(0, n, n);
    expect_reject("robust_wmean out overlaps a source", [&] { robust_wmean({s3[0], lo, s3[2]}, ctl, mid, sh, w3); });
    expect_ok("robust_wmean out beside a source", [&] { robust_wmean({s3[0], lo, s3[2]}, ctl, hi, sh, w3); });
    auto shv = big.narrow(0, n / 2, n / 2).view(bf);
    expect_reject("robust_wmean shadow overlaps a source", [&] { robust_wmean({s3[0], lo, s3[2]}, ctl, out, shv, w3); });

    expect_ok("robust_geomed_finalize row 0", [&] { robust_geomed_finalize(w3, grid, 3, 1e-6, 0, ctl, gs); });
    expect_ok("robust_geomed_finalize last row", [&] { robust_geomed_finalize(w16, grid, 16, 1e-6, 6, ctl, gs); });
    expect_reject("robust_geomed_finalize row past stats", [&] { robust_geomed_finalize(w3, grid, 3, 1e-6, 7, ctl, gs); });
    expect_reject("robust_geomed_finalize iter < 0", [&] { robust_geomed_finalize(w3, grid, 3, 1e-6, -1, ctl, gs); });
    expect_reject("robust_geomed_finalize nu 0", [&] { robust_geomed_finalize(w3, grid, 3, 0.0, 0, ctl, gs); });
    expect_reject("robust_geomed_finalize nu < 0", [&] { robust_geomed_finalize(w3, grid, 3, -1e-6, 0, ctl, gs); });
    expect_reject("robust_geomed_finalize nu NaN", [&] { robust_geomed_finalize(w3, grid, 3, std::nan(""), 0, ctl, gs); });
    expect_reject("robust_geomed_finalize nu inf", [&] { robust_geomed_finalize(w3, grid, 3, HUGE_VAL, 0, ctl, gs); });
    expect_reject("robust_geomed_finalize M 17", [&] { robust_geomed_finalize(w16, grid, 17, 1e-6, 0, ctl, gs); });
    expect_reject("robust_geomed_finalize M past partial", [&] { robust_geomed_finalize(w3, grid, 4, 1e-6, 0, ctl, gs); });
    expect_reject("robust_geomed_finalize grid 4097", [&] { robust_geomed_finalize(w16, 4097, 3, 1e-6, 0, ctl, gs); });
    expect_reject("robust_geomed_finalize short ctl", [&] { robust_geomed_finalize(w3, grid, 3, 1e-6, 0, T_({19}, f32), gs); });
    expect_reject("robust_geomed_finalize stats dtype", [&] { robust_geomed_finalize(w3, grid, 3, 1e-6, 0, ctl, T_({34}, f32)); });
  }
  // ---- client-level privacy: w / anchor fp32, the bf16 shadow, one double per block, 4 stats floats
  {
    const auto f64 = at::kDouble;
    const int64_t n = 4096 * 1024 + 4 * 257;  // the grid-stride loop wraps, ragged last block
    const int64_t grid = fd_privacy_grid(n);
    auto w = T_({n}, f32), a = T_({n}, f32), sh = T_({n}, bf), part = T_({grid}, f64), st = T_({4}, f32);
    const int64_t top = (int64_t(1) << 32) - 1;
    expect_ok("privacy_norm", [&] { privacy_norm(w, a, part, st, 0.5); });
    expect_ok("privacy_apply", [&] { privacy_apply(w, a, sh, st, 0.01, 1, 2, 3, 4, 0); });
    expect_ok("privacy_apply no shadow, sigma 0", [&] { privacy_apply(w, a, none, st, 0.0, 0, 0, 0, 0, 0); });
    expect_ok("privacy_apply top words, first4 past 2^32", [&] {
      privacy_apply(w, a, sh, st, 0.01, top, top, top, top, (int64_t(1) << 32) - 8);
    });
    expect_ok("privacy_gauss", [&] { privacy_gauss(w, 1, 2, 3, 4, 0); });
    auto w8 = T_({2048}, f32), a8 = T_({2048}, f32), p8 = T_({2}, f64);
    expect_ok("privacy_norm small", [&] { privacy_norm(w8, a8, p8, st, 1.0); });
    expect_ok("privacy_apply small", [&] { privacy_apply(w8, a8, none, st, 0.5, 0, 0, 0, 1, 7); });
    auto srt = T_({n - 4}, f32), shs = T_({n - 4}, bf), part_short = T_({grid - 1}, f64), st3 = T_({3}, f32),
         st8 = T_({8}, f32);
    expect_reject("privacy_norm short anchor", [&] { privacy_norm(w, srt, part, st, 0.5); });
    expect_reject("privacy_norm short partial", [&] { privacy_norm(w, a, part_short, st, 0.5); });
    expect_reject("privacy_norm short stats", [&] { privacy_norm(w, a, part, st3, 0.5); });
    expect_reject("privacy_norm long stats", [&] { privacy_norm(w, a, part, st8, 0.5); });
    expect_reject("privacy_apply short anchor", [&] { privacy_apply(w, srt, sh, st, 0.01, 1, 2, 3, 4, 0); });
    expect_reject("privacy_apply short shadow", [&] { privacy_apply(w, a, shs, st, 0.01, 1, 2, 3, 4, 0); });
    expect_reject("privacy_apply short stats", [&] { privacy_apply(w, a, sh, st3, 0.01, 1, 2, 3, 4, 0); });
    auto wb = T_({n}, bf), shf = T_({n}, f32), partf = T_({grid}, f32), std_ = T_({4}, f64);
    expect_reject("privacy_norm w dtype", [&] { privacy_norm(wb, a, part, st, 0.5); });
    expect_reject("privacy_norm anchor dtype", [&] { privacy_norm(w, wb, part, st, 0.5); });
    expect_reject("privacy_norm partial dtype", [&] { privacy_norm(w, a, partf, st, 0.5); });
    expect_reject("privacy_norm stats dtype", [&] { privacy_norm(w, a, part, std_, 0.5); });
    expect_reject("privacy_apply shadow dtype", [&] { privacy_apply(w, a, shf, st, 0.01, 1, 2, 3, 4, 0); });
    expect_reject("privacy_apply stats dtype", [&] { privacy_apply(w, a, sh, std_, 0.01, 1, 2, 3, 4, 0); });
    expect_reject("privacy_gauss dtype", [&] { privacy_gauss(wb, 1, 2, 3, 4, 0); });
    auto xt = T_({2, n / 2}, f32).t();
    expect_reject("privacy_norm non-contiguous", [&] { privacy_norm(xt, a, part, st, 0.5); });
    expect_reject("privacy_apply non-contiguous anchor", [&] { privacy_apply(w, xt, sh, st, 0.01, 1, 2, 3, 4, 0); });
    auto w6 = T_({2046}, f32), a6 = T_({2046}, f32), w0 = T_({0}, f32);
    expect_reject("privacy_norm numel % 4", [&] { privacy_norm(w6, a6, p8, st, 1.0); });
    expect_reject("privacy_apply numel % 4", [&] { privacy_apply(w6, a6, none, st, 0.0, 0, 0, 0, 0, 0); });
    expect_reject("privacy_gauss numel % 4", [&] { privacy_gauss(w6, 0, 0, 0, 0, 0); });
    expect_reject("privacy_gauss empty", [&] { privacy_gauss(w0, 0, 0, 0, 0, 0); });
    const double inf = HUGE_VAL;
    expect_reject("privacy_norm clip 0", [&] { privacy_norm(w, a, part, st, 0.0); });
    expect_reject("privacy_norm clip < 0", [&] { privacy_norm(w, a, part, st, -1.0); });
    expect_reject("privacy_norm clip inf", [&] { privacy_norm(w, a, part, st, inf); });
    expect_reject("privacy_norm clip NaN", [&] { privacy_norm(w, a, part, st, std::nan("")); });
    expect_reject("privacy_norm clip beyond fp32", [&] { privacy_norm(w, a, part, st, 1e300); });
    expect_reject("privacy_norm clip below fp32", [&] { privacy_norm(w, a, part, st, 1e-300); });
    expect_reject("privacy_apply sigma < 0", [&] { privacy_apply(w, a, sh, st, -0.01, 1, 2, 3, 4, 0); });
    expect_reject("privacy_apply sigma inf", [&] { privacy_apply(w, a, sh, st, inf, 1, 2, 3, 4, 0); });
    expect_reject("privacy_apply sigma NaN", [&] { privacy_apply(w, a, sh, st, std::nan(""), 1, 2, 3, 4, 0); });
    expect_reject("privacy_apply round < 0", [&] { privacy_apply(w, a, sh, st, 0.01, 1, 2, -1, 4, 0); });
    expect_reject("privacy_apply client < 0", [&] { privacy_apply(w, a, sh, st, 0.01, 1, 2, 3, -1, 0); });
    expect_reject("privacy_apply first4 < 0", [&] { privacy_apply(w, a, sh, st, 0.01, 1, 2, 3, 4, -1); });
    expect_reject("privacy_apply round 2^32", [&] { privacy_apply(w, a, sh, st, 0.01, 1, 2, top + 1, 4, 0); });
    expect_reject("privacy_apply seed word 2^32", [&] { privacy_apply(w, a, sh, st, 0.01, top + 1, 2, 3, 4, 0); });
    expect_reject("privacy_gauss client < 0", [&] { privacy_gauss(w, 1, 2, 3, -4, 0); });
    expect_reject("privacy_gauss first4 < 0", [&] { privacy_gauss(w, 1, 2, 3, 4, -8); });
    // anchor / shadow as a window of w's allocation
    auto big = T_({2 * n}, f32);
    auto lo = big.narrow(0, 0, n), mid = big.narrow(0, n / 2, n), hi = big.narrow(0, n, n);
    expect_reject("privacy_norm anchor is w", [&] { privacy_norm(w, w, part, st, 0.5); });
    expect_reject("privacy_norm anchor overlaps w", [&] { privacy_norm(lo, mid, part, st, 0.5); });
    expect_ok("privacy_norm anchor beside w", [&] { privacy_norm(lo, hi, part, st, 0.5); });
    expect_reject("privacy_apply anchor overlaps w", [&] { privacy_apply(lo, mid, sh, st, 0.01, 1, 2, 3, 4, 0); });
    expect_ok("privacy_apply anchor beside w", [&] { privacy_apply(lo, hi, sh, st, 0.01, 1, 2, 3, 4, 0); });
    auto shv = big.narrow(0, n / 2, n / 2).view(bf);
    expect_reject("privacy_apply shadow overlaps w", [&] { privacy_apply(lo, a, shv, st, 0.01, 1, 2, 3, 4, 0); });
    expect_reject("privacy_apply shadow overlaps anchor", [&] { privacy_apply(w, lo, shv, st, 0.01, 1, 2, 3, 4, 0); });
  }
  // ---- quantized exchange: w / anchor / residual fp32, the int32 payload, three doubles per block
  {
    const auto f64 = at::kDouble;
    const int64_t n = 4096 * 1024 + 64 * 5;  // the grid-stride loop wraps, ragged last sweep
    const int64_t grid = fd_quant_grid(n), w8 = fd_quant_words(n, 8), w4 = fd_quant_words(n, 4);
    auto w = T_({n}, f32), a = T_({n}, f32), e = T_({n}, f32), sh = T_({n}, bf), out = T_({n}, f32);
    auto p8 = T_({w8}, i32), p4 = T_({w4}, i32), part = T_({3 * grid}, f64), st = T_({4}, f64);
    const int64_t top = (int64_t(1) << 32) - 1;
    if (quant_words(n, 8) != n / 4 + n / 64 || quant_words(n, 4) != n / 8 + n / 64) {
      std::printf("FAIL quant_words: %lld / %lld words\n", (long long)quant_words(n, 8), (long long)quant_words(n, 4));
      ++failures;
    }
    expect_ok("quant_encode int8", [&] { quant_encode(w, a, e, p8, part, st, 8, false, 1, 2, 3, 4, 0); });
    expect_ok("quant_encode int4 stochastic, no residual", [&] { quant_encode(w, a, none, p4, part, st, 4, true, 1, 2, 3, 4, 0); });
    expect_ok("quant_encode top words, first past 2^32", [&] {
      quant_encode(w, a, e, p8, part, st, 8, true, top, top, top, top, (int64_t(1) << 32) + 5);
    });
    std::vector<at::Tensor> m8(16), m4(16);
    for (int s = 0; s < 16; ++s) { m8[s] = T_({w8}, i32); m4[s] = T_({w4}, i32); }
    expect_ok("quant_decode_mean M 1", [&] { quant_decode_mean({p8}, a, out, sh, 8); });
    expect_ok("quant_decode_mean M 16", [&] { quant_decode_mean(m8, a, out, sh, 8); });
    expect_ok("quant_decode_mean int4 M 16, no shadow", [&] { quant_decode_mean(m4, a, out, none, 4); });
    expect_ok("quant_decode_mean M 3", [&] { quant_decode_mean({m4[0], m4[1], p4}, a, out, sh, 4); });
    auto ws = T_({2048}, f32), as = T_({2048}, f32), ps = T_({2048 / 4 + 32}, i32), p3 = T_({6}, f64);
    expect_ok("quant_encode small", [&] { quant_encode(ws, as, none, ps, p3, st, 8, false, 0, 0, 0, 0, 7); });
    expect_ok("quant_decode_mean small", [&] { quant_decode_mean({ps}, as, ws, none, 8); });
    // extents
    auto srt = T_({n - 64}, f32), shs = T_({n - 64}, bf), p8s = T_({w8 - 1}, i32), p8l = T_({w8 + 1}, i32);
    auto part_short = T_({3 * grid - 1}, f64), st3 = T_({3}, f64), st8 = T_({8}, f64);
    expect_reject("quant_encode short anchor", [&] { quant_encode(w, srt, e, p8, part, st, 8, false, 1, 2, 3, 4, 0); });
    expect_reject("quant_encode short residual", [&] { quant_encode(w, a, srt, p8, part, st, 8, false, 1, 2, 3, 4, 0); });
    expect_reject("quant_encode short payload", [&] { quant_encode(w, a, e, p8s, part, st, 8, false, 1, 2, 3, 4, 0); });
    expect_reject("quant_encode long payload", [&] { quant_encode(w, a, e, p8l, part, st, 8, false, 1, 2, 3, 4, 0); });
    expect_reject("quant_encode int4 payload at int8", [&] { quant_encode(w, a, e, p4, part, st, 8, false, 1, 2, 3, 4, 0); });
    expect_reject("quant_encode int8 payload at int4", [&] { quant_encode(w, a, e, p8, part, st, 4, false, 1, 2, 3, 4, 0); });
    expect_reject("quant_encode short partial", [&] { quant_encode(w, a, e, p8, part_short, st, 8, false, 1, 2, 3, 4, 0); });
    expect_reject("quant_encode short stats", [&] { quant_encode(w, a, e, p8, part, st3, 8, false, 1, 2, 3, 4, 0); });
    expect_reject("quant_encode long stats", [&] { quant_encode(w, a, e, p8, part, st8, 8, false, 1, 2, 3, 4, 0); });
    expect_reject("quant_decode_mean short payload", [&] { quant_decode_mean({m8[0], p8s}, a, out, sh, 8); });
    expect_reject("quant_decode_mean short anchor", [&] { quant_decode_mean({p8}, srt, out, sh, 8); });
    expect_reject("quant_decode_mean short shadow", [&] { quant_decode_mean({p8}, a, out, shs, 8); });
    expect_reject("quant_decode_mean int4 payload at int8", [&] { quant_decode_mean({p4}, a, out, sh, 8); });
    // dtypes, layout
    auto wb = T_({n}, bf), shf = T_({n}, f32), p8f = T_({w8}, f32), partf = T_({3 * grid}, f32), stf = T_({4}, f32);
    expect_reject("quant_encode w dtype", [&] { quant_encode(wb, a, e, p8, part, st, 8, false, 1, 2, 3, 4, 0); });
    expect_reject("quant_encode anchor dtype", [&] { quant_encode(w, wb, e, p8, part, st, 8, false, 1, 2, 3, 4, 0); });
    expect_reject("quant_encode residual dtype", [&] { quant_encode(w, a, wb, p8, part, st, 8, false, 1, 2, 3, 4, 0); });
    expect_reject("quant_encode payload dtype", [&] { quant_encode(w, a, e, p8f, part, st, 8, false, 1, 2, 3, 4, 0); });
    expect_reject("quant_encode partial dtype", [&] { quant_encode(w, a, e, p8, partf, st, 8, false, 1, 2, 3, 4, 0); });
    expect_reject("quant_encode stats dtype", [&] { quant_encode(w, a, e, p8, part, stf, 8, false, 1, 2, 3, 4, 0); });
    expect_reject("quant_decode_mean payload dtype", [&] { quant_decode_mean({p8f}, a, out, sh, 8); });
    expect_reject("quant_decode_mean out dtype", [&] { quant_decode_mean({p8}, a, wb, sh, 8); });
    expect_reject("quant_decode_mean shadow dtype", [&] { quant_decode_mean({p8}, a, out, shf, 8); });
    auto xt = T_({2, n / 2}, f32).t();
    expect_reject("quant_encode non-contiguous", [&] { quant_encode(xt, a, e, p8, part, st, 8, false, 1, 2, 3, 4, 0); });
    expect_reject("quant_decode_mean non-contiguous anchor", [&] { quant_decode_mean({p8}, xt, out, sh, 8); });
    // lengths, widths, counts, streams
    auto w60 = T_({2044}, f32), a60 = T_({2044}, f32), w0 = T_({0}, f32), p0 = T_({0}, i32);
    expect_reject("quant_encode numel % 64", [&] { quant_encode(w60, a60, none, ps, p3, st, 8, false, 0, 0, 0, 0, 0); });
    expect_reject("quant_encode empty", [&] { quant_encode(w0, w0, none, p0, p3, st, 8, false, 0, 0, 0, 0, 0); });
    expect_reject("quant_decode_mean numel % 64", [&] { quant_decode_mean({ps}, a60, w60, none, 8); });
    expect_reject("quant_words numel % 64", [&] { quant_words(100, 8); });
    expect_reject("quant_words bits", [&] { quant_words(128, 16); });
    expect_reject("quant_encode bits 2", [&] { quant_encode(w, a, e, p8, part, st, 2, false, 1, 2, 3, 4, 0); });
    expect_reject("quant_encode bits 16", [&] { quant_encode(w, a, e, p8, part, st, 16, false, 1, 2, 3, 4, 0); });
    expect_reject("quant_decode_mean bits 0", [&] { quant_decode_mean({p8}, a, out, sh, 0); });
    expect_reject("quant_decode_mean M 0", [&] { quant_decode_mean({}, a, out, sh, 8); });
    std::vector<at::Tensor> m17(m8);
    m17.push_back(p8);
    expect_reject("quant_decode_mean M 17", [&] { quant_decode_mean(m17, a, out, sh, 8); });
    expect_reject("quant_encode round < 0", [&] { quant_encode(w, a, e, p8, part, st, 8, true, 1, 2, -1, 4, 0); });
    expect_reject("quant_encode client < 0", [&] { quant_encode(w, a, e, p8, part, st, 8, true, 1, 2, 3, -1, 0); });
    expect_reject("quant_encode first < 0", [&] { quant_encode(w, a, e, p8, part, st, 8, true, 1, 2, 3, 4, -1); });
    expect_reject("quant_encode round 2^32", [&] { quant_encode(w, a, e, p8, part, st, 8, true, 1, 2, top + 1, 4, 0); });
    expect_reject("quant_encode seed word 2^32", [&] { quant_encode(w, a, e, p8, part, st, 8, true, top + 1, 2, 3, 4, 0); });
    expect_reject("quant_encode first overflows", [&] {
      quant_encode(w, a, e, p8, part, st, 8, true, 1, 2, 3, 4, std::numeric_limits<int64_t>::max() / 16);
    });
    // windows of one allocation
    auto big = T_({2 * n}, f32);
    auto lo = big.narrow(0, 0, n), mid = big.narrow(0, n / 2, n), hi = big.narrow(0, n, n);
    expect_reject("quant_encode anchor is w", [&] { quant_encode(w, w, e, p8, part, st, 8, false, 1, 2, 3, 4, 0); });
    expect_reject("quant_encode residual is w", [&] { quant_encode(w, a, w, p8, part, st, 8, false, 1, 2, 3, 4, 0); });
    expect_reject("quant_encode anchor overlaps w", [&] { quant_encode(lo, mid, e, p8, part, st, 8, false, 1, 2, 3, 4, 0); });
    expect_reject("quant_encode residual overlaps anchor", [&] { quant_encode(w, lo, mid, p8, part, st, 8, false, 1, 2, 3, 4, 0); });
    expect_ok("quant_encode anchor beside w", [&] { quant_encode(lo, hi, e, p8, part, st, 8, false, 1, 2, 3, 4, 0); });
    auto pv8 = big.narrow(0, n / 2, w8).view(i32);
    expect_reject("quant_encode payload overlaps w", [&] { quant_encode(lo, a, e, pv8, part, st, 8, false, 1, 2, 3, 4, 0); });
    expect_reject("quant_encode payload overlaps residual", [&] { quant_encode(w, a, lo, pv8, part, st, 8, false, 1, 2, 3, 4, 0); });
    expect_reject("quant_decode_mean out is anchor", [&] { quant_decode_mean({p8}, a, a, sh, 8); });
    expect_reject("quant_decode_mean out overlaps anchor", [&] { quant_decode_mean({p8}, mid, lo, sh, 8); });
    expect_ok("quant_decode_mean out beside anchor", [&] { quant_decode_mean({p8}, hi, lo, sh, 8); });
    expect_reject("quant_decode_mean out overlaps a payload", [&] { quant_decode_mean({m8[0], pv8}, a, lo, sh, 8); });
    auto shv = big.narrow(0, n / 2, n / 2).view(bf);
    expect_reject("quant_decode_mean shadow overlaps out", [&] { quant_decode_mean({p8}, a, lo, shv, 8); });
    expect_reject("quant_decode_mean shadow overlaps anchor", [&] { quant_decode_mean({p8}, lo, out, shv, 8); });
    expect_reject("quant_decode_mean shadow overlaps a payload", [&] { quant_decode_mean({pv8}, a, out, shv, 8); });
  }
  // ---- top-k sparsified exchange: w / anchor / residual fp32, the int32 payload, the byte workspace
  {
    const auto f64 = at::kDouble, u8 = at::kByte;
    const int64_t n = 4096 * 1024 + 3 * 4096 + 64 * 5;  // the chunk loops wrap, ragged last chunk
    const int64_t k = n / 100, kh = n / 2;
    const int64_t wk = fd_topk_words(n, k), w1 = fd_topk_words(n, 1), wh = fd_topk_words(n, kh), wb = fd_topk_work_bytes(n);
    auto w = T_({n}, f32), a = T_({n}, f32), e = T_({n}, f32), sh = T_({n}, bf), out = T_({n}, f32);
    auto pk = T_({wk}, i32), p1 = T_({w1}, i32), ph = T_({wh}, i32), work = T_({wb}, u8), st = T_({8}, f64);
    if (topk_words(n, k) != (n + 4095) / 4096 + 1 + k + (k + 1) / 2 || topk_words(64, 1) != 4 || topk_grid(n) != 1024 ||
        topk_grid(64) != 1 || topk_work_bytes(n) != wb || wb < n * 4) {
      std::printf("FAIL topk_words / topk_grid / topk_work_bytes\n");
      ++failures;
    }
    expect_ok("topk_encode", [&] { topk_encode(w, a, e, pk, work, st, k); });
    expect_ok("topk_encode no residual", [&] { topk_encode(w, a, none, pk, work, st, k); });
    expect_ok("topk_encode k 1", [&] { topk_encode(w, a, e, p1, work, st, 1); });
    expect_ok("topk_encode k n / 2", [&] { topk_encode(w, a, e, ph, work, st, kh); });
    std::vector<at::Tensor> mk(16);
    for (int s = 0; s < 16; ++s) mk[s] = T_({wk}, i32);
    expect_ok("topk_decode_mean M 1", [&] { topk_decode_mean({pk}, a, out, sh, k); });
    expect_ok("topk_decode_mean M 16", [&] { topk_decode_mean(mk, a, out, sh, k); });
    expect_ok("topk_decode_mean M 16, no shadow", [&] { topk_decode_mean(mk, a, out, none, k); });
    expect_ok("topk_decode_mean k 1", [&] { topk_decode_mean({p1}, a, out, sh, 1); });
    expect_ok("topk_decode_mean k n / 2", [&] { topk_decode_mean({ph, ph}, a, out, none, kh); });
    // the smallest n: one ragged chunk of 64
    auto ws = T_({64}, f32), as = T_({64}, f32), es = T_({64}, f32), ps = T_({fd_topk_words(64, 32)}, i32);
    auto works = T_({fd_topk_work_bytes(64)}, u8), p1s = T_({4}, i32);
    expect_ok("topk_encode n 64, k n / 2", [&] { topk_encode(ws, as, es, ps, works, st, 32); });
    expect_ok("topk_encode n 64, k 1, no residual", [&] { topk_encode(ws, as, none, p1s, works, st, 1); });
    expect_ok("topk_decode_mean n 64", [&] { topk_decode_mean({ps}, as, ws, none, 32); });
    // extents
    auto srt = T_({n - 64}, f32), shs = T_({n - 64}, bf), pks = T_({wk - 1}, i32), pkl = T_({wk + 1}, i32);
    auto work_short = T_({wb - 1}, u8), st7 = T_({7}, f64), st9 = T_({9}, f64);
    expect_reject("topk_encode short anchor", [&] { topk_encode(w, srt, e, pk, work, st, k); });
    expect_reject("topk_encode short residual", [&] { topk_encode(w, a, srt, pk, work, st, k); });
    expect_reject("topk_encode short payload", [&] { topk_encode(w, a, e, pks, work, st, k); });
    expect_reject("topk_encode long payload", [&] { topk_encode(w, a, e, pkl, work, st, k); });
    expect_reject("topk_encode payload of another k", [&] { topk_encode(w, a, e, pk, work, st, k + 1); });
    expect_reject("topk_encode short work", [&] { topk_encode(w, a, e, pk, work_short, st, k); });
    expect_reject("topk_encode short stats", [&] { topk_encode(w, a, e, pk, work, st7, k); });
    expect_reject("topk_encode long stats", [&] { topk_encode(w, a, e, pk, work, st9, k); });
    auto work_odd = T_({wb + 16}, u8).narrow(0, 4, wb);
    expect_reject("topk_encode misaligned work", [&] { topk_encode(w, a, e, pk, work_odd, st, k); });
    expect_reject("topk_decode_mean short payload", [&] { topk_decode_mean({mk[0], pks}, a, out, sh, k); });
    expect_reject("topk_decode_mean payload of another k", [&] { topk_decode_mean({p1}, a, out, sh, k); });
    expect_reject("topk_decode_mean short anchor", [&] { topk_decode_mean({pk}, srt, out, sh, k); });
    expect_reject("topk_decode_mean short shadow", [&] { topk_decode_mean({pk}, a, out, shs, k); });
    // dtypes, layout
    auto wbf = T_({n}, bf), shf = T_({n}, f32), pkf = T_({wk}, f32), workf = T_({wb / 4 + 4}, f32), stf = T_({8}, f32);
    expect_reject("topk_encode w dtype", [&] { topk_encode(wbf, a, e, pk, work, st, k); });
    expect_reject("topk_encode anchor dtype", [&] { topk_encode(w, wbf, e, pk, work, st, k); });
    expect_reject("topk_encode residual dtype", [&] { topk_encode(w, a, wbf, pk, work, st, k); });
    expect_reject("topk_encode payload dtype", [&] { topk_encode(w, a, e, pkf, work, st, k); });
    expect_reject("topk_encode work dtype", [&] { topk_encode(w, a, e, pk, workf, st, k); });
    expect_reject("topk_encode stats dtype", [&] { topk_encode(w, a, e, pk, work, stf, k); });
    expect_reject("topk_decode_mean payload dtype", [&] { topk_decode_mean({pkf}, a, out, sh, k); });
    expect_reject("topk_decode_mean out dtype", [&] { topk_decode_mean({pk}, a, wbf, sh, k); });
    expect_reject("topk_decode_mean shadow dtype", [&] { topk_decode_mean({pk}, a, out, shf, k); });
    auto xt = T_({2, n / 2}, f32).t();
    expect_reject("topk_encode non-contiguous", [&] { topk_encode(xt, a, e, pk, work, st, k); });
    expect_reject("topk_decode_mean non-contiguous anchor", [&] { topk_decode_mean({pk}, xt, out, sh, k); });
    // lengths, k, counts
    auto w60 = T_({2044}, f32), a60 = T_({2044}, f32), w0 = T_({0}, f32), p0 = T_({0}, i32);
    expect_reject("topk_encode numel % 64", [&] { topk_encode(w60, a60, none, ps, works, st, 32); });
    expect_reject("topk_encode empty", [&] { topk_encode(w0, w0, none, p0, works, st, 1); });
    expect_reject("topk_decode_mean numel % 64", [&] { topk_decode_mean({ps}, a60, w60, none, 32); });
    expect_reject("topk_words numel % 64", [&] { topk_words(100, 1); });
    expect_reject("topk_words numel 2^31", [&] { topk_words(int64_t(1) << 31, 1); });
    expect_reject("topk_words k 0", [&] { topk_words(128, 0); });
    expect_reject("topk_words k above n / 2", [&] { topk_words(128, 65); });
    expect_reject("topk_work_bytes numel % 64", [&] { topk_work_bytes(100); });
    expect_reject("topk_encode k 0", [&] { topk_encode(w, a, e, pk, work, st, 0); });
    expect_reject("topk_encode k < 0", [&] { topk_encode(w, a, e, pk, work, st, -1); });
    expect_reject("topk_encode k above n / 2", [&] { topk_encode(w, a, e, ph, work, st, kh + 1); });
    expect_reject("topk_decode_mean k 0", [&] { topk_decode_mean({pk}, a, out, sh, 0); });
    expect_reject("topk_decode_mean k above n / 2", [&] { topk_decode_mean({ph}, a, out, sh, kh + 1); });
    expect_reject("topk_decode_mean M 0", [&] { topk_decode_mean({}, a, out, sh, k); });
    std::vector<at::Tensor> m17(mk);
    m17.push_back(pk);
    expect_reject("topk_decode_mean M 17", [&] { topk_decode_mean(m17, a, out, sh, k); });
    // windows of one allocation
    auto big = T_({2 * n}, f32);
    auto lo = big.narrow(0, 0, n), mid = big.narrow(0, n / 2, n), hi = big.narrow(0, n, n);
    expect_reject("topk_encode anchor is w", [&] { topk_encode(w, w, e, pk, work, st, k); });
    expect_reject("topk_encode residual is w", [&] { topk_encode(w, a, w, pk, work, st, k); });
    expect_reject("topk_encode anchor overlaps w", [&] { topk_encode(lo, mid, e, pk, work, st, k); });
    expect_reject("topk_encode residual overlaps anchor", [&] { topk_encode(w, lo, mid, pk, work, st, k); });
    expect_ok("topk_encode anchor beside w", [&] { topk_encode(lo, hi, e, pk, work, st, k); });
    auto pvk = big.narrow(0, n / 2, wk).view(i32);
    auto workv = big.narrow(0, n / 2, wb / 4).view(u8);
    expect_reject("topk_encode payload overlaps w", [&] { topk_encode(lo, a, e, pvk, work, st, k); });
    expect_reject("topk_encode payload overlaps residual", [&] { topk_encode(w, a, lo, pvk, work, st, k); });
    expect_reject("topk_encode work overlaps w", [&] { topk_encode(lo, a, e, pk, workv, st, k); });
    expect_reject("topk_encode work overlaps residual", [&] { topk_encode(w, a, hi, pk, workv, st, k); });
    expect_reject("topk_decode_mean out is anchor", [&] { topk_decode_mean({pk}, a, a, sh, k); });
    expect_reject("topk_decode_mean out overlaps anchor", [&] { topk_decode_mean({pk}, mid, lo, sh, k); });
    expect_ok("topk_decode_mean out beside anchor", [&] { topk_decode_mean({pk}, hi, lo, sh, k); });
    expect_reject("topk_decode_mean out overlaps a payload", [&] { topk_decode_mean({mk[0], pvk}, a, lo, sh, k); });
    auto shv = big.narrow(0, n / 2, n / 2).view(bf);
    expect_reject("topk_decode_mean shadow overlaps out", [&] { topk_decode_mean({pk}, a, lo, shv, k); });
    expect_reject("topk_decode_mean shadow overlaps anchor", [&] { topk_decode_mean({pk}, lo, out, shv, k); });
    expect_reject("topk_decode_mean shadow overlaps a payload", [&] { topk_decode_mean({pvk}, a, out, shv, k); });
  }
  // ---- secure aggregation: w / anchor fp32, the int32 keys [P, 8], the int32 payload of n + 16 words,
  // four doubles per block
  {
    const auto f64 = at::kDouble;
    const int64_t n = 2048 * 1024 + 16 * 5;  // the grid-stride loop wraps, ragged last sweep
    const int64_t grid = fd_secagg_grid(n), words = fd_secagg_words(n);
    auto w = T_({n}, f32), a = T_({n}, f32), sh = T_({n}, bf), out = T_({n}, f32), so = T_({n}, i32);
    auto k0 = T_({0, 8}, i32), k1 = T_({1, 8}, i32), k15 = T_({15, 8}, i32), key = T_({8}, i32);
    auto p = T_({words}, i32), part = T_({4 * grid}, f64), st = T_({4}, f64);
    const int64_t top = (int64_t(1) << 32) - 1;
    if (secagg_words(n) != n + 16 || secagg_grid(n) != 2048 || secagg_grid(16) != 1) {
      std::printf("FAIL secagg_words / secagg_grid\n");
      ++failures;
    }
    expect_ok("secagg_stream", [&] { secagg_stream(so, key, {1, 2, 3}, 20, 0); });
    expect_ok("secagg_stream 8 rounds, top nonce, last blocks", [&] {
      secagg_stream(so, key, {top, top, top}, 8, (int64_t(1) << 32) - n / 16);
    });
    expect_ok("secagg_mask P 0", [&] { secagg_mask(w, a, k0, 0, p, part, st, 24, 20, 0, 0); });
    expect_ok("secagg_mask P 1", [&] { secagg_mask(w, a, k1, 1, p, part, st, 8, 12, 7, 5); });
    expect_ok("secagg_mask P 15, top round, last blocks", [&] {
      secagg_mask(w, a, k15, 0x7fff, p, part, st, 30, 8, top, (int64_t(1) << 32) - n / 16 - 1);
    });
    std::vector<at::Tensor> m16(16);
    for (int s = 0; s < 16; ++s) m16[s] = T_({words}, i32);
    expect_ok("secagg_unmask_mean M 1", [&] { secagg_unmask_mean({p}, a, out, sh, 24); });
    expect_ok("secagg_unmask_mean M 16", [&] { secagg_unmask_mean(m16, a, out, sh, 24); });
    expect_ok("secagg_unmask_mean M 3, no shadow", [&] { secagg_unmask_mean({m16[0], m16[1], p}, a, out, none, 8); });
    auto rows = T_({3, words}, i32);
    expect_ok("secagg_unmask_mean rows of a gather", [&] {
      secagg_unmask_mean({rows.select(0, 0), rows.select(0, 2)}, a, out, sh, 24);
    });
    auto ws = T_({16}, f32), as = T_({16}, f32), ps = T_({32}, i32), p4 = T_({4}, f64);
    expect_ok("secagg_mask small", [&] { secagg_mask(ws, as, k1, 0, ps, p4, st, 24, 20, 0, 0); });
    expect_ok("secagg_unmask_mean small", [&] { secagg_unmask_mean({ps}, as, ws, none, 24); });
    // extents
    auto srt = T_({n - 16}, f32), shs = T_({n - 16}, bf), psh = T_({words - 1}, i32), pl = T_({words + 1}, i32);
    auto pn = T_({n}, i32), part_short = T_({4 * grid - 1}, f64), st3 = T_({3}, f64), st8 = T_({8}, f64);
    auto k16 = T_({16, 8}, i32), k7w = T_({1, 7}, i32), kflat = T_({8}, i32), key7 = T_({7}, i32);
    expect_reject("secagg_mask short anchor", [&] { secagg_mask(w, srt, k1, 0, p, part, st, 24, 20, 0, 0); });
    expect_reject("secagg_mask short payload", [&] { secagg_mask(w, a, k1, 0, psh, part, st, 24, 20, 0, 0); });
    expect_reject("secagg_mask long payload", [&] { secagg_mask(w, a, k1, 0, pl, part, st, 24, 20, 0, 0); });
    expect_reject("secagg_mask payload without the check block", [&] { secagg_mask(w, a, k1, 0, pn, part, st, 24, 20, 0, 0); });
    expect_reject("secagg_mask short partial", [&] { secagg_mask(w, a, k1, 0, p, part_short, st, 24, 20, 0, 0); });
    expect_reject("secagg_mask short stats", [&] { secagg_mask(w, a, k1, 0, p, part, st3, 24, 20, 0, 0); });
    expect_reject("secagg_mask long stats", [&] { secagg_mask(w, a, k1, 0, p, part, st8, 24, 20, 0, 0); });
    expect_reject("secagg_mask 16 partners", [&] { secagg_mask(w, a, k16, 0, p, part, st, 24, 20, 0, 0); });
    expect_reject("secagg_mask keys of 7 words", [&] { secagg_mask(w, a, k7w, 0, p, part, st, 24, 20, 0, 0); });
    expect_reject("secagg_mask flat keys", [&] { secagg_mask(w, a, kflat, 0, p, part, st, 24, 20, 0, 0); });
    expect_reject("secagg_mask a sign bit beyond P", [&] { secagg_mask(w, a, k1, 2, p, part, st, 24, 20, 0, 0); });
    expect_reject("secagg_mask signs < 0", [&] { secagg_mask(w, a, k1, -1, p, part, st, 24, 20, 0, 0); });
    expect_reject("secagg_stream short key", [&] { secagg_stream(so, key7, {1, 2, 3}, 20, 0); });
    expect_reject("secagg_stream nonce of 2 words", [&] { secagg_stream(so, key, {1, 2}, 20, 0); });
    expect_reject("secagg_unmask_mean short payload", [&] { secagg_unmask_mean({m16[0], psh}, a, out, sh, 24); });
    expect_reject("secagg_unmask_mean payload without the check block", [&] { secagg_unmask_mean({pn}, a, out, sh, 24); });
    expect_reject("secagg_unmask_mean short anchor", [&] { secagg_unmask_mean({p}, srt, out, sh, 24); });
    expect_reject("secagg_unmask_mean short shadow", [&] { secagg_unmask_mean({p}, a, out, shs, 24); });
    // dtypes
    auto wb = T_({n}, bf), pf = T_({words}, f32), partf = T_({4 * grid}, f32), stf = T_({4}, f32), shf = T_({n}, f32);
    auto k1f = T_({1, 8}, f32), k1l = T_({1, 8}, i64);
    expect_reject("secagg_mask w dtype", [&] { secagg_mask(wb, a, k1, 0, p, part, st, 24, 20, 0, 0); });
    expect_reject("secagg_mask anchor dtype", [&] { secagg_mask(w, wb, k1, 0, p, part, st, 24, 20, 0, 0); });
    expect_reject("secagg_mask keys dtype", [&] { secagg_mask(w, a, k1f, 0, p, part, st, 24, 20, 0, 0); });
    expect_reject("secagg_mask keys int64", [&] { secagg_mask(w, a, k1l, 0, p, part, st, 24, 20, 0, 0); });
    expect_reject("secagg_mask payload dtype", [&] { secagg_mask(w, a, k1, 0, pf, part, st, 24, 20, 0, 0); });
    expect_reject("secagg_mask partial dtype", [&] { secagg_mask(w, a, k1, 0, p, partf, st, 24, 20, 0, 0); });
    expect_reject("secagg_mask stats dtype", [&] { secagg_mask(w, a, k1, 0, p, part, stf, 24, 20, 0, 0); });
    expect_reject("secagg_stream out dtype", [&] { secagg_stream(w, key, {1, 2, 3}, 20, 0); });
    expect_reject("secagg_stream key dtype", [&] { secagg_stream(so, k1f, {1, 2, 3}, 20, 0); });
    expect_reject("secagg_unmask_mean payload dtype", [&] { secagg_unmask_mean({pf}, a, out, sh, 24); });
    expect_reject("secagg_unmask_mean out dtype", [&] { secagg_unmask_mean({p}, a, wb, sh, 24); });
    expect_reject("secagg_unmask_mean shadow dtype", [&] { secagg_unmask_mean({p}, a, out, shf, 24); });
    // contiguity
    auto xt = T_({2, n / 2}, f32).t();
    expect_reject("secagg_mask non-contiguous", [&] { secagg_mask(xt, a, k1, 0, p, part, st, 24, 20, 0, 0); });
    expect_reject("secagg_unmask_mean non-contiguous anchor", [&] { secagg_unmask_mean({p}, xt, out, sh, 24); });
    expect_reject("secagg_mask non-contiguous keys", [&] {
      secagg_mask(w, a, T_({8, 2}, i32).t(), 0, p, part, st, 24, 20, 0, 0);
    });
    // values
    auto w24 = T_({24}, f32), a24 = T_({24}, f32), p40 = T_({40}, i32), w0 = T_({0}, f32), p16 = T_({16}, i32);
    auto so24 = T_({24}, i32), so0 = T_({0}, i32);
    expect_reject("secagg_mask numel % 16", [&] { secagg_mask(w24, a24, k1, 0, p40, p4, st, 24, 20, 0, 0); });
    expect_reject("secagg_mask empty", [&] { secagg_mask(w0, w0, k1, 0, p16, p4, st, 24, 20, 0, 0); });
    expect_reject("secagg_stream numel % 16", [&] { secagg_stream(so24, key, {1, 2, 3}, 20, 0); });
    expect_reject("secagg_stream empty", [&] { secagg_stream(so0, key, {1, 2, 3}, 20, 0); });
    expect_reject("secagg_unmask_mean numel % 16", [&] { secagg_unmask_mean({p40}, a24, w24, none, 24); });
    expect_reject("secagg_words numel % 16", [&] { secagg_words(100); });
    expect_reject("secagg_mask frac_bits 7", [&] { secagg_mask(w, a, k1, 0, p, part, st, 7, 20, 0, 0); });
    expect_reject("secagg_mask frac_bits 31", [&] { secagg_mask(w, a, k1, 0, p, part, st, 31, 20, 0, 0); });
    expect_reject("secagg_mask 10 rounds", [&] { secagg_mask(w, a, k1, 0, p, part, st, 24, 10, 0, 0); });
    expect_reject("secagg_mask 0 rounds", [&] { secagg_mask(w, a, k1, 0, p, part, st, 24, 0, 0, 0); });
    expect_reject("secagg_stream 16 rounds", [&] { secagg_stream(so, key, {1, 2, 3}, 16, 0); });
    expect_reject("secagg_unmask_mean frac_bits 7", [&] { secagg_unmask_mean({p}, a, out, sh, 7); });
    expect_reject("secagg_unmask_mean frac_bits 31", [&] { secagg_unmask_mean({p}, a, out, sh, 31); });
    expect_reject("secagg_unmask_mean M 0", [&] { secagg_unmask_mean({}, a, out, sh, 24); });
    std::vector<at::Tensor> m17(m16);
    m17.push_back(p);
    expect_reject("secagg_unmask_mean M 17", [&] { secagg_unmask_mean(m17, a, out, sh, 24); });
    expect_reject("secagg_mask round < 0", [&] { secagg_mask(w, a, k1, 0, p, part, st, 24, 20, -1, 0); });
    expect_reject("secagg_mask round 2^32", [&] { secagg_mask(w, a, k1, 0, p, part, st, 24, 20, top + 1, 0); });
    expect_reject("secagg_mask first_block < 0", [&] { secagg_mask(w, a, k1, 0, p, part, st, 24, 20, 0, -1); });
    expect_reject("secagg_mask the check block's counter is 2^32", [&] {
      secagg_mask(w, a, k1, 0, p, part, st, 24, 20, 0, (int64_t(1) << 32) - n / 16);
    });
    expect_reject("secagg_mask first_block overflows", [&] {
      secagg_mask(w, a, k1, 0, p, part, st, 24, 20, 0, std::numeric_limits<int64_t>::max());
    });
    expect_reject("secagg_stream first_block < 0", [&] { secagg_stream(so, key, {1, 2, 3}, 20, -1); });
    expect_reject("secagg_stream the last counter is 2^32", [&] {
      secagg_stream(so, key, {1, 2, 3}, 20, (int64_t(1) << 32) - n / 16 + 1);
    });
    expect_reject("secagg_stream nonce word < 0", [&] { secagg_stream(so, key, {1, -2, 3}, 20, 0); });
    expect_reject("secagg_stream nonce word 2^32", [&] { secagg_stream(so, key, {1, 2, top + 1}, 20, 0); });
    // windows of one allocation
    auto big = T_({2 * n + 32}, f32);
    auto lo = big.narrow(0, 0, n), mid = big.narrow(0, n / 2, n), hi = big.narrow(0, n, n);
    expect_reject("secagg_mask anchor is w", [&] { secagg_mask(w, w, k1, 0, p, part, st, 24, 20, 0, 0); });
    expect_reject("secagg_mask anchor overlaps w", [&] { secagg_mask(lo, mid, k1, 0, p, part, st, 24, 20, 0, 0); });
    expect_ok("secagg_mask anchor beside w", [&] { secagg_mask(lo, hi, k1, 0, p, part, st, 24, 20, 0, 0); });
    auto pv = big.narrow(0, n / 2, words).view(i32);
    expect_reject("secagg_mask payload overlaps w", [&] { secagg_mask(lo, a, k1, 0, pv, part, st, 24, 20, 0, 0); });
    expect_reject("secagg_mask payload overlaps anchor", [&] { secagg_mask(w, lo, k1, 0, pv, part, st, 24, 20, 0, 0); });
    auto kv = big.narrow(0, 8, 8).view(i32).view({1, 8});
    expect_reject("secagg_mask keys inside w", [&] { secagg_mask(lo, a, kv, 0, p, part, st, 24, 20, 0, 0); });
    expect_reject("secagg_mask a misaligned w", [&] {
      secagg_mask(big.narrow(0, 1, n), a, k1, 0, p, part, st, 24, 20, 0, 0);
    });
    expect_reject("secagg_stream key inside out", [&] { secagg_stream(pv, pv.narrow(0, 16, 8), {1, 2, 3}, 20, 0); });
    expect_reject("secagg_unmask_mean out is anchor", [&] { secagg_unmask_mean({p}, a, a, sh, 24); });
    expect_reject("secagg_unmask_mean out overlaps anchor", [&] { secagg_unmask_mean({p}, mid, lo, sh, 24); });
    expect_ok("secagg_unmask_mean out beside anchor", [&] { secagg_unmask_mean({p}, hi, lo, sh, 24); });
    expect_reject("secagg_unmask_mean out overlaps a payload", [&] { secagg_unmask_mean({m16[0], pv}, a, lo, sh, 24); });
    auto shv = big.narrow(0, n / 2, n / 2).view(bf);
    expect_reject("secagg_unmask_mean shadow overlaps out", [&] { secagg_unmask_mean({p}, a, lo, shv, 24); });
    expect_reject("secagg_unmask_mean shadow overlaps anchor", [&] { secagg_unmask_mean({p}, lo, out, shv, 24); });
    expect_reject("secagg_unmask_mean shadow overlaps a payload", [&] { secagg_unmask_mean({pv}, a, out, shv, 24); });
  }
  // ---- embedding backward (work = pieces + LayerNorm partials)
  {
    const int64_t Tn = 2688, D = 768, V = 1000, P = 512;
    auto dy = T_({Tn, D}, bf), ids = T_({Tn}, i64), srt = T_({Tn}, i64), prm = T_({Tn}, i64);
    auto word = T_({V, D}, bf), pos = T_({P, D}, bf), ga = T_({D}, f32), mean = T_({Tn}, f32), rstd = T_({Tn}, f32);
    auto dword = T_({V, D}, f32), dpos = T_({P, D}, f32), dg = T_({D}, f32), db = T_({D}, f32), dz = T_({Tn, D}, f32);
    auto work = T_({Tn * D + 256 * 3 * D}, f32), work_small = T_({Tn * D}, f32), seed = T_({1}, i32);
    expect_ok("emb bwd", [&] { emb_bwd(dy, ids, srt, prm, word, pos, ga, mean, rstd, dword, dpos, dg, db, dz, work,
                                       128, seed, 1, 0, 1.0, false, none, none, none, none); });
    expect_reject("emb bwd work", [&] { emb_bwd(dy, ids, srt, prm, word, pos, ga, mean, rstd, dword, dpos, dg, db, dz,
                                                work_small, 128, seed, 1, 0, 1.0, false, none, none, none, none); });
    // the backward's deferred column sums riding on the tail launch
    auto part = T_({21 * 3 * D}, f32), part_small = T_({20 * 3 * D}, f32);
    std::vector<std::vector<c10::optional<at::Tensor>>> outs = {{dg, db, c10::optional<at::Tensor>(T_({D}, f32))}};
    expect_ok("emb bwd + colsum jobs", [&] { emb_bwd(dy, ids, srt, prm, word, pos, ga, mean, rstd, dword, dpos, dg, db,
                                                     dz, work, 128, seed, 1, 0, 1.0, false, none, none, none, none,
                                                     {part}, outs, {21}, {3 * D}, {D}, {0}); });
    expect_reject("emb bwd colsum part", [&] { emb_bwd(dy, ids, srt, prm, word, pos, ga, mean, rstd, dword, dpos, dg,
                                                       db, dz, work, 128, seed, 1, 0, 1.0, false, none, none, none,
                                                       none, {part_small}, outs, {21}, {3 * D}, {D}, {0}); });
  }
  // ---- unpadded layout
  {
    auto mask = T_({32, 128}, i64), ids = T_({32, 128}, i64), rm = T_({2688}, i32), cu = T_({33}, i32);
    auto ip = T_({2688}, i64);
    expect_ok("pack", [&] { pack(mask, ids, rm, cu, ip, none, none, none, none); });
    {
      auto ga = T_({300, 768}, bf), gb = T_({300, 768}, bf), go = T_({64, 768}, bf), go2 = T_({64, 768}, bf);
      auto gi = T_({64}, i64);
      expect_ok("gather_rows2", [&] { gather_rows2(ga, gb, go, go2, gi); });
      expect_ok("scatter_rows2", [&] { scatter_rows2(go, go2, ga, gb, gi, 32); });
      auto gbad = T_({63, 768}, bf);
      expect_reject("gather_rows2 shapes", [&] { gather_rows2(ga, gb, gbad, go2, gi); });
      expect_reject("scatter_rows2 nsrc", [&] { scatter_rows2(go, go2, ga, gb, gi, 65); });
    }
    auto st1 = T_({1}, i32);
    expect_ok("pack + counters", [&] { pack(mask, ids, rm, cu, ip, st1, st1, none, none); });
    auto stf = T_({1}, f32);
    expect_reject("pack counter dtype", [&] { pack(mask, ids, rm, cu, ip, stf, none, none, none); });
    auto cu_bad = T_({32}, i32);
    expect_reject("pack cu", [&] { pack(mask, ids, rm, cu_bad, ip, none, none, none, none); });
  }
  if (failures) {
    std::printf("binding host check: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("binding host check: ok (%d launcher calls validated)\n", hc::calls);
  return 0;
}
