// Transformer encoder runtime (BERT / XLM-R): replaces the remote embedding server reached through
// litellm.embedding() (super_rag/llm/embed/embedding_service.py:168-175) and the remote
// cross-encoder reached through litellm.arerank() (super_rag/llm/rerank/rerank_service.py:95-104).
//
// Per layer (post-LN BERT block), all on one HIP stream:
//   qkv  = GEMM(h16, Wqkv) + bqkv                 fp16  [M, 3d]     (K4, bias epilogue)
//   ctx  = MHA(qkv, mask)                         fp16  [M, d]      (K5)
//   y32  = GEMM(ctx, Wo) + bo + h32               fp32  [M, d]      (K4, residual epilogue)
//   h    = LayerNorm(y32)                         fp16 + fp32       (K6)
//   f    = GELU(GEMM(h16, W1) + b1)               fp16  [M, F]      (K4, GELU epilogue)
//   y32  = GEMM(f, W2) + b2 + h32                 fp32              (K4, residual epilogue)
//   h    = LayerNorm(y32)                         fp16 + fp32       (K6)
// The residual stream is fp32 by default (fp16 residuals cost ~2x the embedding error,
// DESIGN.md); cross-encoders may run it in fp16 (config.residual_fp16).  With CLS pooling or a
// classification head the last layer is computed for the CLS rows only.
// Embedding mode pools (CLS / masked mean) and L2-normalises (K7); cross-encoder mode applies the
// RoBERTa classification head: tanh(GEMM(h16[CLS rows], Wc) + bc) (fp32) . Wout + bout (K4 + K8).
// With a token-heads request (forward_dev's TokenHeads) the last layer runs for every token and the
// final states also feed the sparse head (sparse_token_weights, sparse_terms) and / or the
// multi-vector head (a bias GEMM, then colbert_pack), per chunk (k_encoder_misc.hip).
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "sr_kernels.h"
#include "sr_runtime.h"

namespace sr {

Encoder::Encoder(const sr_encoder_config& cfg, int device) : cfg_(cfg), device_(device) {
  const int d = cfg.hidden;
  SR_CHECK(cfg.vocab_size > 0 && d > 0 && cfg.layers > 0 && cfg.heads > 0 &&
               cfg.intermediate > 0 && cfg.max_position > 0 && cfg.type_vocab > 0,
           "encoder: config fields must be positive");
  SR_CHECK(d % cfg.heads == 0 && (d / cfg.heads == 64 || d / cfg.heads == 32),
           "encoder: head dim must be 32 or 64");
  SR_CHECK(d % 128 == 0 && cfg.intermediate % 128 == 0,
           "encoder: hidden and intermediate must be multiples of 128");
  SR_CHECK(d <= 2048, "encoder: hidden must be <= 2048");
  SR_CHECK(cfg.classifier == 0 || (cfg.classifier == 1 && cfg.num_labels >= 1),
           "encoder: classifier must be 0 or 1 (with num_labels >= 1)");
  max_tokens_ = cfg.max_tokens > 0 ? cfg.max_tokens : 262144;
  DeviceGuard g(device_);
  SR_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
  SR_HIP(hipEventCreateWithFlags(&done_, hipEventDisableTiming));

  const int64_t D = d, F = cfg.intermediate;
  {
    // split weights for the DEEP fp32-residual embedders only: measured against the fp32 oracle
    // (tools/embed_split_error.py), the 24-layer bge-m3 needs them (1.07e-3 max relative error
    // without, 5.3e-4 with; bar 1e-3), the 12-layer bge-base does not (6.1e-4 without, 4.1e-4
    // with) and embeds 1.5x faster without (B = 256: 4.28 -> 2.86 ms).  SR_WEIGHT_SPLIT = 0 / 1
    // forces the choice.
    const char* e = std::getenv("SR_WEIGHT_SPLIT");
    const bool deep = cfg.layers > 12;
    split_ = !cfg.residual_fp16 && (e && e[0] ? e[0] != '0' : deep);
  }
  const int64_t sk = split_ ? D : 0, skf = split_ ? F : 0;
  register_target("embeddings.word_embeddings.weight", wemb_, (int64_t)cfg.vocab_size * D, true);
  register_target("embeddings.position_embeddings.weight", pemb_, (int64_t)cfg.max_position * D, true);
  register_target("embeddings.token_type_embeddings.weight", temb_, (int64_t)cfg.type_vocab * D, true);
  register_target("embeddings.LayerNorm.weight", embg_, D, false);
  register_target("embeddings.LayerNorm.bias", embb_, D, false);
  layers_.resize(cfg.layers);
  for (int l = 0; l < cfg.layers; ++l) {
    Layer& L = layers_[l];
    const std::string p = "encoder.layer." + std::to_string(l) + ".";
    register_target(p + "attention.self.query.weight", L.wqkv, D * D, true, 0, 3 * D * D, sk);
    register_target(p + "attention.self.key.weight", L.wqkv, D * D, true, D * D, 3 * D * D, sk);
    register_target(p + "attention.self.value.weight", L.wqkv, D * D, true, 2 * D * D, 3 * D * D, sk);
    register_target(p + "attention.self.query.bias", L.bqkv, D, false, 0, 3 * D);
    register_target(p + "attention.self.key.bias", L.bqkv, D, false, D, 3 * D);
    register_target(p + "attention.self.value.bias", L.bqkv, D, false, 2 * D, 3 * D);
    register_target(p + "attention.output.dense.weight", L.wo, D * D, true, 0, -1, sk);
    register_target(p + "attention.output.dense.bias", L.bo, D, false);
    register_target(p + "attention.output.LayerNorm.weight", L.ln1g, D, false);
    register_target(p + "attention.output.LayerNorm.bias", L.ln1b, D, false);
    register_target(p + "intermediate.dense.weight", L.w1, F * D, true, 0, -1, sk);
    register_target(p + "intermediate.dense.bias", L.b1, F, false);
    register_target(p + "output.dense.weight", L.w2, D * F, true, 0, -1, skf);
    register_target(p + "output.dense.bias", L.b2, D, false);
    register_target(p + "output.LayerNorm.weight", L.ln2g, D, false);
    register_target(p + "output.LayerNorm.bias", L.ln2b, D, false);
  }
  // fp32 masters of the weights that LayerNorm folding rescales (fp16 residual stream only)
  if (cfg.residual_fp16) {
    for (int l = 0; l < cfg.layers; ++l) {
      Layer& L = layers_[l];
      const std::string p = "encoder.layer." + std::to_string(l) + ".";
      L.wqkv32.reserve((size_t)3 * D * D * sizeof(float));
      L.w132.reserve((size_t)F * D * sizeof(float));
      targets_[p + "attention.self.query.weight"].master = L.wqkv32.as<float>();
      targets_[p + "attention.self.key.weight"].master = L.wqkv32.as<float>() + D * D;
      targets_[p + "attention.self.value.weight"].master = L.wqkv32.as<float>() + 2 * D * D;
      targets_[p + "intermediate.dense.weight"].master = L.w132.as<float>();
    }
  }
  if (cfg.classifier == 1) {
    register_target("classifier.dense.weight", wc_, D * D, true);
    register_target("classifier.dense.bias", bc_, D, false);
    register_target("classifier.out_proj.weight", wout_, (int64_t)cfg.num_labels * D, false);
    register_target("classifier.out_proj.bias", bout_, cfg.num_labels, false);
  }
}

Encoder::~Encoder() {
  (void)hipSetDevice(device_);
  if (done_) {
    (void)hipEventSynchronize(done_);
    (void)hipEventDestroy(done_);
  }
  if (stream_) {
    (void)hipStreamSynchronize(stream_);
    (void)hipStreamDestroy(stream_);
  }
}

void Encoder::register_target(const std::string& name, DevBuf& buf, int64_t numel, bool f16,
                              int64_t offset_elems, int64_t total_elems, int64_t split_k) {
  const int64_t total = total_elems < 0 ? numel : total_elems;
  const size_t esz = f16 ? sizeof(half_t) : sizeof(float);
  const int64_t rep = split_k > 0 ? 2 : 1;  // split: hi and lo halves of every row
  if (buf.p == nullptr) {
    buf.reserve((size_t)total * rep * esz);
    SR_HIP(hipMemset(buf.p, 0, (size_t)total * rep * esz));
  }
  Target t{reinterpret_cast<char*>(buf.p) + offset_elems * rep * esz, numel, f16};
  t.split_k = split_k;
  targets_[name] = t;
  is_set_[name] = false;
}

void Encoder::set_weight(const std::string& name, const float* data, int64_t numel) {
  if (name == "sparse_linear.weight" || name == "sparse_linear.bias") {
    // the optional sparse head, kept fp32; never part of missing() / sr_encoder_ready
    const bool is_w = name == "sparse_linear.weight";
    const int64_t want = is_w ? cfg_.hidden : 1;
    SR_CHECK(numel == want, "encoder: weight '" + name + "' has " + std::to_string(numel) +
                                " elements, expected " + std::to_string(want));
    SR_CHECK(data != nullptr, "encoder: null weight data");
    DeviceGuard g(device_);
    begin(stream_);
    SR_HIP(hipStreamSynchronize(stream_));
    DevBuf& buf = is_w ? sparse_w_ : sparse_b_;
    buf.reserve((size_t)want * sizeof(float));
    SR_HIP(hipMemcpy(buf.p, data, (size_t)want * sizeof(float), hipMemcpyHostToDevice));
    (is_w ? sparse_w_set_ : sparse_b_set_) = true;
    return;
  }
  if (name == "colbert_linear.weight" || name == "colbert_linear.bias") {
    // the optional multi-vector head: W [dc, hidden] fp16 (the GEMM's W layout), bias [dc] fp32;
    // dc comes from the weight's count.  Never part of missing() / sr_encoder_ready
    const bool is_w = name == "colbert_linear.weight";
    SR_CHECK(data != nullptr, "encoder: null weight data");
    if (is_w) {
      const int64_t dc = numel / cfg_.hidden;
      SR_CHECK(numel > 0 && numel % cfg_.hidden == 0 && dc % 128 == 0 && dc <= 1024,
               "encoder: weight '" + name + "' has " + std::to_string(numel) +
                   " elements, expected dc * hidden with dc a multiple of 128, <= 1024");
    } else {
      // the weight defines dc: the bias follows it
      if (!colbert_w_set_) throw Error(SR_ERR_STATE, "encoder: weight not set: colbert_linear.weight");
      SR_CHECK(numel == colbert_dc_, "encoder: weight '" + name + "' has " + std::to_string(numel) +
                                         " elements, expected " + std::to_string(colbert_dc_));
    }
    DeviceGuard g(device_);
    begin(stream_);
    SR_HIP(hipStreamSynchronize(stream_));
    if (is_w) {
      std::vector<half_t> h((size_t)numel);
      for (int64_t i = 0; i < numel; ++i) h[i] = (half_t)data[i];
      colbert_w_.reserve(h.size() * sizeof(half_t));
      SR_HIP(hipMemcpy(colbert_w_.p, h.data(), h.size() * sizeof(half_t), hipMemcpyHostToDevice));
      if (colbert_dc_ != (int)(numel / cfg_.hidden)) colbert_b_set_ = false;  // a head of another width
      colbert_dc_ = (int)(numel / cfg_.hidden);
      colbert_w_set_ = true;
    } else {
      colbert_b_.reserve((size_t)numel * sizeof(float));
      SR_HIP(hipMemcpy(colbert_b_.p, data, (size_t)numel * sizeof(float), hipMemcpyHostToDevice));
      colbert_b_set_ = true;
    }
    return;
  }
  auto it = targets_.find(name);
  SR_CHECK(it != targets_.end(), "encoder: unknown weight '" + name + "'");
  const Target& t = it->second;
  SR_CHECK(numel == t.numel, "encoder: weight '" + name + "' has " + std::to_string(numel) +
                                 " elements, expected " + std::to_string(t.numel));
  SR_CHECK(data != nullptr, "encoder: null weight data");
  DeviceGuard g(device_);
  begin(stream_);
  SR_HIP(hipStreamSynchronize(stream_));
  if (t.f16 && t.split_k > 0) {  // row r -> [fp16(w) | fp16(w - fp16(w))], 2 split_k halfs
    const int64_t K = t.split_k;
    SR_CHECK(numel % K == 0, "encoder: split weight '" + name + "' is not whole rows");
    std::vector<half_t> h((size_t)numel * 2);
    for (int64_t r = 0; r < numel / K; ++r)
      for (int64_t j = 0; j < K; ++j) {
        const float v = data[r * K + j];
        const half_t hi = (half_t)v;
        h[(size_t)(r * 2 * K + j)] = hi;
        h[(size_t)(r * 2 * K + K + j)] = (half_t)(v - (float)hi);
      }
    SR_HIP(hipMemcpy(t.ptr, h.data(), h.size() * sizeof(half_t), hipMemcpyHostToDevice));
  } else if (t.f16) {
    std::vector<half_t> h((size_t)numel);
    for (int64_t i = 0; i < numel; ++i) h[i] = (half_t)data[i];
    SR_HIP(hipMemcpy(t.ptr, h.data(), (size_t)numel * sizeof(half_t), hipMemcpyHostToDevice));
  } else {
    SR_HIP(hipMemcpy(t.ptr, data, (size_t)numel * sizeof(float), hipMemcpyHostToDevice));
  }
  if (t.master)
    SR_HIP(hipMemcpy(t.master, data, (size_t)numel * sizeof(float), hipMemcpyHostToDevice));
  is_set_[name] = true;
  fold_ready_ = false;
}

// an A/B switch of the environment: on unless set to 0
static bool switch_on(const char* name) {
  const char* e = std::getenv(name);
  return !(e && e[0] == '0');
}

// LayerNorm folding: with an fp16 residual stream the two LayerNorms of a block are
// never materialised.  The GEMM that produces a residual sum u also writes per-row Chan partial
// statistics; the next GEMM consumes u itself with LN(u) = (u - mu) rstd gamma + beta folded in:
//   LN(u) . W^T + b = rstd (u . (W diag gamma)^T - mu c) + (W beta + b),  c[n] = sum_k W'[n][k],
// and the residual epilogues rebuild LN(u) element-wise.  SR_LN_FOLD=0 disables it (A/B tests).
bool Encoder::fold_enabled() const {
  if (!cfg_.residual_fp16) return false;
  if (cfg_.hidden % 256 != 0 || cfg_.intermediate % 256 != 0) return false;
  return switch_on("SR_LN_FOLD");
}

// K5c (fused QKV projection + attention) for the folded layers at S == 128; SR_FUSED_QKV_ATTN=0
// keeps the QKV GEMM + K5b pair (bit-identical results; A/B tests).  Same-box bench: 461.2 vs
// 454.3 q/s (profiles/r02_fused_qkv_attention/).
static bool fused_qkv_attention_enabled() { return switch_on("SR_FUSED_QKV_ATTN"); }

// K/V-free CLS-only last layer of the folded cross-encoders (cls_attn_fold, k_encoder_misc.hip):
// no K / V projection of the S tokens; SR_KVFREE_CLS=0 keeps the K, V GEMM + CLS attention (A/B).
static bool kvfree_cls_enabled() { return switch_on("SR_KVFREE_CLS"); }

// The fp8 modes (sr_runtime.h, set_fp8) as the GEMMs of a folded layer that run in fp8
Encoder::Fp8Plan Encoder::fp8_plan(int mode) {
  SR_CHECK((mode >= 0 && mode <= 3) || (SR_WITH_DIAG && mode >= 4 && mode <= 5),
           "encoder: fp8 mode must be 0 .. 3 (modes 4 / 5 were rejected: diagnostic library only)");
  Fp8Plan p;
  p.ffn2 = mode >= 1;
  p.ffn1 = mode >= 2;
  p.qkv = mode == 2 || mode == 4;
  p.qkv_norm = mode == 4;
  p.oproj = mode == 5;
  return p;
}

void Encoder::set_fp8(int mode) {
  const Fp8Plan p = fp8_plan(mode);
  if (p.ffn2) {  // every fp8 mode runs FFN2 (K = intermediate) in fp8; the others have K = hidden
    SR_CHECK(fold_enabled(), "encoder: fp8 modes need the LN-folded fp16-residual path");
    SR_CHECK(cfg_.intermediate % 128 == 0 && cfg_.intermediate >= 256 &&
                 (!(p.ffn1 || p.qkv || p.oproj) || (cfg_.hidden % 128 == 0 && cfg_.hidden >= 256)),
             "encoder: fp8 GEMMs need K % 128 == 0, K >= 256");
  }
  if (mode != fp8_) {
    fp8_ = mode;
    plan_ = p;
    fold_ready_ = false;  // re-derive the folded weights (and their e4m3 copies)
  }
}

// The folded weights serve every S: prepare_fold asks for the K/V-free form at the rerank pair
// length (hidden and heads decide it; forward_dev asks again with the S it runs)
static constexpr int kKvfreePrepS = 128;

void Encoder::prepare_fold(hipStream_t s) {
  if (fold_ready_) return;
  const int64_t D = cfg_.hidden, F = cfg_.intermediate;
  for (size_t l = 0; l < layers_.size(); ++l) {
    Layer& L = layers_[l];
    L.w1_f.reserve((size_t)F * D * sizeof(half_t));
    L.c1.reserve((size_t)F * sizeof(float));
    L.d1.reserve((size_t)F * sizeof(float));
    launch_fold_ln_weight(L.w132.as<float>(), L.ln1g.as<float>(), L.ln1b.as<float>(),
                          L.b1.as<float>(), (int)F, (int)D, L.w1_f.as<half_t>(), L.c1.as<float>(),
                          L.d1.as<float>(), s);
    L.w2h.reserve((size_t)D * F * sizeof(half_t));  // 0.5 W2: FFN1 stores 2 GELU (exact scale)
    launch_scale_f16(L.w2.as<half_t>(), 0.5f, L.w2h.as<half_t>(), D * F, s);
    if (plan_.ffn2) {
      L.w2_8.reserve((size_t)D * F);
      L.w2e.reserve((size_t)D);
      launch_quantize_rows_fp8(L.w2h.as<half_t>(), (int)D, (int)F, L.w2_8.as<uint8_t>(),
                               L.w2e.as<uint8_t>(), s);
    }
    if (plan_.ffn1) {
      L.w1_8.reserve((size_t)F * D);
      L.w1e.reserve((size_t)F);
      L.c1_8.reserve((size_t)F * sizeof(float));
      launch_quantize_rows_fp8(L.w1_f.as<half_t>(), (int)F, (int)D, L.w1_8.as<uint8_t>(),
                               L.w1e.as<uint8_t>(), s);
      launch_colsum_fp8(L.w1_8.as<uint8_t>(), L.w1e.as<uint8_t>(), (int)F, (int)D,
                        L.c1_8.as<float>(), s);
    }
    if (plan_.oproj) {
      L.wo_8.reserve((size_t)D * D);
      L.woe.reserve((size_t)D);
      launch_quantize_rows_fp8(L.wo.as<half_t>(), (int)D, (int)D, L.wo_8.as<uint8_t>(),
                               L.woe.as<uint8_t>(), s);
    }
    L.b2_f.reserve((size_t)D * sizeof(float));  // FFN2 bias + beta of LN1 (rebuilt residual)
    launch_vec_add(L.b2.as<float>(), L.ln1b.as<float>(), L.b2_f.as<float>(), (int)D, s);
    if (l == 0) continue;  // layer 0 reads the (normalised) embedding LayerNorm output
    const Layer& P = layers_[l - 1];
    const bool kvfree_prep = l + 1 == layers_.size() && kvfree_cls_enabled() &&
                             cls_attn_fold_supported(kKvfreePrepS, (int)D, cfg_.heads);
    L.bo_f.reserve((size_t)D * sizeof(float));  // O-proj bias + beta of the previous LN2
    launch_vec_add(L.bo.as<float>(), P.ln2b.as<float>(), L.bo_f.as<float>(), (int)D, s);
    L.wqkv_f.reserve((size_t)3 * D * D * sizeof(half_t));
    L.cqkv.reserve((size_t)3 * D * sizeof(float));
    L.dqkv.reserve((size_t)3 * D * sizeof(float));
    launch_fold_ln_weight(L.wqkv32.as<float>(), P.ln2g.as<float>(), P.ln2b.as<float>(),
                          L.bqkv.as<float>(), (int)(3 * D), (int)D, L.wqkv_f.as<half_t>(),
                          L.cqkv.as<float>(), L.dqkv.as<float>(), s);
    if (kvfree_prep) {
      const int64_t HD = (int64_t)cfg_.heads * D;
      L.wk_bd.reserve((size_t)HD * D * sizeof(half_t));
      L.wv_bd.reserve((size_t)D * 2 * HD * sizeof(half_t));
      L.zb.reserve((size_t)HD * sizeof(float));
      SR_HIP(hipMemsetAsync(L.zb.p, 0, (size_t)HD * sizeof(float), s));
      launch_kv_blockdiag(L.wqkv_f.as<half_t>(), (int)D, cfg_.heads, L.wk_bd.as<half_t>(),
                          L.wv_bd.as<half_t>(), s);
    }
    if (plan_.qkv) {
      L.wqkv8.reserve((size_t)3 * D * D);
      L.wqkve.reserve((size_t)3 * D);
      L.cqkv8.reserve((size_t)3 * D * sizeof(float));
      launch_quantize_rows_fp8(L.wqkv_f.as<half_t>(), (int)(3 * D), (int)D, L.wqkv8.as<uint8_t>(),
                               L.wqkve.as<uint8_t>(), s);
      launch_colsum_fp8(L.wqkv8.as<uint8_t>(), L.wqkve.as<uint8_t>(), (int)(3 * D), (int)D,
                        L.cqkv8.as<float>(), s);
    }
  }
  if (plan_.qkv_norm) {  // (mu, rstd) = (0, 1) for every row: this QKV reads normalised rows
    unit_mr_.reserve(2 * sizeof(float));
    const float one[2] = {0.f, 1.f};
    SR_HIP(hipMemcpyAsync(unit_mr_.p, one, sizeof(one), hipMemcpyHostToDevice, s));
    SR_HIP(hipStreamSynchronize(s));
  }
  fold_ready_ = true;
}

std::string Encoder::missing() const {
  for (const auto& kv : is_set_)
    if (!kv.second) return kv.first;
  return std::string();
}

void Encoder::ensure_ws(int64_t tokens) {
  if (tokens <= ws_tokens_) return;
  SR_HIP(hipEventSynchronize(done_));  // the previous call may still use the old workspace
  const int64_t d = cfg_.hidden, F = cfg_.intermediate;
  ids_.reserve((size_t)tokens * sizeof(int32_t));
  mask_.reserve((size_t)tokens * sizeof(int32_t));
  types_.reserve((size_t)tokens * sizeof(int32_t));
  pos_.reserve((size_t)tokens * sizeof(int32_t));
  h16_.reserve((size_t)tokens * d * sizeof(half_t));
  h32_.reserve((size_t)tokens * d * sizeof(float));
  qkv_.reserve((size_t)tokens * 3 * d * sizeof(half_t));
  ctx_.reserve((size_t)tokens * d * sizeof(half_t));
  y32_.reserve((size_t)tokens * d * sizeof(float));
  ffn_.reserve((size_t)tokens * F * sizeof(half_t));
  u8_.reserve((size_t)tokens * d);
  // split-K partial tiles of the short-M GEMMs (launch_gemm: LnFold.chunk_ws), a fixed 64 MiB
  if (!fold_enabled()) chunk_ws_.reserve(kChunkWsBytes);
  if (cfg_.residual_fp16) {
    statA_.reserve((size_t)tokens * (d / 128 + 1) * 2 * sizeof(float));
    statB_.reserve((size_t)tokens * (d / 128 + 1) * 2 * sizeof(float));
    mrA_.reserve((size_t)tokens * 2 * sizeof(float));
    mrB_.reserve((size_t)tokens * 2 * sizeof(float));
  }
  ws_tokens_ = tokens;
}

void Encoder::check_forward(int B, int S, int mode, int pool, int out_dtype, int ld_out,
                            const TokenHeads* heads) const {
  SR_CHECK(B >= 0 && S >= 1, "encoder: bad batch shape");
  const SparseOut* sparse = heads ? heads->sparse : nullptr;
  const MultiVecOut* mv = heads ? heads->multivec : nullptr;
  SR_CHECK(!heads || sparse || mv, "encoder: an empty token-heads request");
  if (mv) {
    SR_CHECK(mode == 0, "encoder: the multi-vector head belongs to the embedding forward");
    SR_CHECK(B == 0 || (mv->vecs && mv->len), "encoder: null multi-vector output");
  }
  if (sparse) {
    SR_CHECK(mode == 0, "encoder: the sparse head belongs to the embedding forward");
    sparse_terms_check_args(B, S, sparse->n_special);
    SR_CHECK(sparse->n_special == 0 || sparse->special_ids, "encoder: null special_ids");
    SR_CHECK(B == 0 || (sparse->terms && sparse->weights && sparse->count), "encoder: null sparse output");
  }
  SR_CHECK(S <= cfg_.max_position - std::max(cfg_.position_offset, 0) - (cfg_.position_offset > 0 ? 1 : 0),
           "encoder: sequence longer than the position table");
  SR_CHECK(mode == 0 || cfg_.classifier == 1, "encoder: model has no classification head");
  SR_CHECK(pool == SR_POOL_CLS || pool == SR_POOL_MEAN, "encoder: pool must be CLS or MEAN");
  SR_CHECK(out_dtype == SR_DTYPE_F32 || out_dtype == SR_DTYPE_F16, "encoder: bad output dtype");
  SR_CHECK(mode == 1 || ld_out >= cfg_.hidden, "encoder: ld_out must be >= hidden");
  const std::string miss = missing();
  if (!miss.empty()) throw Error(SR_ERR_STATE, "encoder: weight not set: " + miss);
  if (sparse && !(sparse_w_set_ && sparse_b_set_))
    throw Error(SR_ERR_STATE, std::string("encoder: weight not set: sparse_linear.") +
                                  (sparse_w_set_ ? "bias" : "weight"));
  if (mv && !(colbert_w_set_ && colbert_b_set_))
    throw Error(SR_ERR_STATE, std::string("encoder: weight not set: colbert_linear.") +
                                  (colbert_w_set_ ? "bias" : "weight"));
  if (mv) colbert_pack_check_args(B, S, colbert_dc_);
}

// The workspaces of one call with launch chunks of chunk_seqs sequences; returns where the sparse
// head's token weights go.  A buffer that has to grow first waits for done_: the previous call may
// still use the old one.
float* Encoder::reserve_forward(int B, int S, int mode, int64_t chunk_seqs, const TokenHeads* heads) {
  const SparseOut* sparse = heads ? heads->sparse : nullptr;
  ensure_ws(chunk_seqs * S);
  if (mode == 1) {
    const size_t need = (size_t)chunk_seqs * cfg_.hidden * sizeof(float);
    if (clst_.bytes < need) SR_HIP(hipEventSynchronize(done_));
    clst_.reserve(need);
  }
  float* tok_weight = sparse ? sparse->tok_weight : nullptr;
  if (sparse && !tok_weight) {
    if (sparse_tw_.bytes < (size_t)B * S * sizeof(float)) SR_HIP(hipEventSynchronize(done_));
    sparse_tw_.reserve((size_t)B * S * sizeof(float));
    tok_weight = sparse_tw_.as<float>();
  }
  if (heads && heads->multivec) {  // the head's GEMM output of one launch chunk
    const size_t need = (size_t)chunk_seqs * S * colbert_dc_ * sizeof(half_t);
    if (colbert_v_.bytes < need) SR_HIP(hipEventSynchronize(done_));
    colbert_v_.reserve(need);
  }
  return tok_weight;
}

void Encoder::forward_dev(const int32_t* ids, const int32_t* mask, const int32_t* types, int B,
                          int S, int mode, int pool, void* out, int out_dtype, int ld_out,
                          hipStream_t s, const TokenHeads* heads) {
  check_forward(B, S, mode, pool, out_dtype, ld_out, heads);
  if (B == 0) return;
  DeviceGuard g(device_);
  // s == nullptr is the HIP null stream (torch's default stream): use it as-is.
  begin(s);
  const int d = cfg_.hidden, H = cfg_.heads;
  const int64_t seqs_per_chunk = std::max<int64_t>(1, max_tokens_ / S);
  float* tok_weight = reserve_forward(B, S, mode, std::min<int64_t>(B, seqs_per_chunk), heads);
  const bool fold = fold_enabled();
  if (fold) prepare_fold(s);

  Chunk c{};
  c.S = S;
  c.s = s;
  // Only the first token's final state is consumed (CLS pooling / classification head): the last
  // layer runs attention for query row 0 only and its O-projection, LayerNorms and FFN on the
  // B CLS rows (exact: every other row of the last layer is dead).
  // The token heads read every token's final state: their request keeps the full last layer.
  c.cls_only = !heads && ((mode == 1) || (pool == SR_POOL_CLS));
  if (fold) {
    c.U = h16_.as<half_t>();
    c.Uc = y32_.as<half_t>();
    c.sA = statA_.as<float>();
    c.sB = statB_.as<float>();
    c.mA = mrA_.as<float>();
    c.mB = mrB_.as<float>();
    c.u8 = u8_.as<uint8_t>();
    // K5c: QKV projection + attention in one kernel (the QKV activation stays in LDS); an fp8 QKV
    // projection runs unfused
    c.fuse_qa = fused_qkv_attention_enabled() && !plan_.qkv && qkv_attention_supported(S, d, H);
    // the fused layers' ctx as e4m3 (in the FFN buffer, dead until this layer's FFN1) and their
    // O-projection on the fp8 MFMA
    c.o8 = plan_.oproj && c.fuse_qa;
    c.ctx8 = ffn_.as<uint8_t>();
    // (an fp8 QKV projection keeps the e4m3 QKV path in every layer)
    c.kvfree = c.cls_only && !plan_.qkv && kvfree_cls_enabled() && layers_.size() > 1 &&
               cls_attn_fold_supported(S, d, H) && layers_.back().wk_bd.p != nullptr;
  }
  for (int64_t b0 = 0; b0 < B; b0 += seqs_per_chunk) {
    c.b0 = b0;
    c.nb = (int)std::min<int64_t>(seqs_per_chunk, B - b0);
    c.M = c.nb * S;
    c.ids = ids + b0 * S;
    c.mask = mask + b0 * S;
    c.types = types ? types + b0 * S : nullptr;
    embed_stage(c);
    if (fold) folded_stack(c);
    else unfolded_stack(c);
    output_stage(c, mode, pool, out, out_dtype, ld_out, heads, tok_weight);
  }
  end(s);
}

void Encoder::embed_stage(const Chunk& c) {
  int32_t* pos = pos_.as<int32_t>();
  launch_positions(c.ids, pos, c.nb, c.S, cfg_.position_offset, c.s);
  launch_embed_ln(c.ids, pos, c.types, wemb_.as<half_t>(), pemb_.as<half_t>(), temb_.as<half_t>(),
                  embg_.as<float>(), embb_.as<float>(), cfg_.ln_eps, c.M, cfg_.hidden, cfg_.vocab_size,
                  cfg_.max_position, cfg_.type_vocab, h16_.as<half_t>(),
                  cfg_.residual_fp16 ? nullptr : h32_.as<float>(), c.s);
}

// The LN-folded layers (fp16 residual stream).  Per layer: QKV + attention -> ctx; O-projection +
// residual -> u1 and its row statistics (sA -> mA); FFN1, FFN2 + residual -> u2 and its statistics
// (sB -> mB).  In a CLS-only last layer the last two run on the nb CLS rows, compact in Uc.
void Encoder::folded_stack(const Chunk& c) {
  for (size_t l = 0; l < layers_.size(); ++l) {
    const bool last = c.cls_only && l + 1 == layers_.size();
    fold_qkv_attention(c, l, last);
    fold_oproj(c, l, last);
    fold_ffn(c, l, last);
  }
  // final LayerNorm (LN2 of the last block) of the rows that are consumed -> h16
  const Layer& Lz = layers_.back();
  launch_ln_apply(c.cls_only ? c.Uc : c.U, cfg_.hidden, c.mB, Lz.ln2g.as<float>(), Lz.ln2b.as<float>(),
                  c.cls_only ? c.nb : c.M, cfg_.hidden, h16_.as<half_t>(), c.s);
}

// ctx of layer l from U, the previous block's u2 (layer 0: the embedding LayerNorm's output), with
// that block's LN2 folded into W'qkv
void Encoder::fold_qkv_attention(const Chunk& c, size_t l, bool last) {
  const Layer& L = layers_[l];
  const int d = cfg_.hidden, H = cfg_.heads, S = c.S, nb = c.nb, M = c.M;
  half_t* U = c.U;
  float* mB = c.mB;
  half_t* qkv = qkv_.as<half_t>();
  half_t* ctx = ctx_.as<half_t>();
  hipStream_t s = c.s;
  LnFold lq;  // A = u of the previous block, its LN2 folded into W'
  lq.mr = mB;
  lq.colsum = L.cqkv.as<float>();
  LnFold lc = lq;  // A = row b*S of each sequence (stride S*d), its statistics at row b*S
  lc.stat_ld = S;
  if (c.fuse_qa && !last) {
    if (l == 0)
      launch_qkv_attention(EPI_BIAS_F16, U, d, L.wqkv.as<half_t>(), L.bqkv.as<float>(), nullptr,
                           c.mask, ctx, nb, S, d, H, s, c.o8 ? c.ctx8 : nullptr);
    else
      launch_qkv_attention(EPI_LNF_F16, U, d, L.wqkv_f.as<half_t>(), L.dqkv.as<float>(), &lq,
                           c.mask, ctx, nb, S, d, H, s, c.o8 ? c.ctx8 : nullptr);
    return;  // K5c ran the attention too
  }
  if (l == 0) {
    launch_gemm(EPI_BIAS_F16, U, d, L.wqkv.as<half_t>(), L.bqkv.as<float>(), nullptr, 0, qkv,
                3 * d, M, 3 * d, d, s);
  } else if (plan_.qkv) {  // A = e4m3 copy of u (by the previous FFN2) or, qkv_norm, of the
                           // normalised rows (quantize_norm_fp8, (mu, rstd) = (0, 1))
    LnFold l8;
    l8.mr = plan_.qkv_norm ? unit_mr_.as<float>() : mB;
    l8.stat_ld = plan_.qkv_norm ? 0 : 1;
    l8.colsum = L.cqkv8.as<float>();
    l8.wexp = L.wqkve.as<uint8_t>();
    launch_gemm_f8w(EPI_LNF_F16, c.u8, d, L.wqkv8.as<uint8_t>(), L.dqkv.as<float>(), nullptr, 0,
                    qkv, 3 * d, M, 3 * d, d, s, &l8);
  } else if (last && c.kvfree) {
    // K/V-free CLS-only last layer: q of the CLS rows, w_h = W'_{k,h}^T q_h (one GEMM on the
    // block-diagonal weight), scores / softmax / z' per sequence (as an fp16 hi + lo pair),
    // ctx = W'_v z' + d_v (one GEMM, K = 2 H d)
    const int64_t HD = (int64_t)H * d;
    half_t* qc = ffn_.as<half_t>();
    half_t* wq = qc + (int64_t)nb * d;
    half_t* zq = wq + (int64_t)nb * HD;
    launch_gemm(EPI_LNF_F16, U, (int64_t)S * d, L.wqkv_f.as<half_t>(), L.dqkv.as<float>(), nullptr,
                0, qc, d, nb, d, d, s, &lc);
    launch_gemm(EPI_BIAS_F16, qc, d, L.wk_bd.as<half_t>(), L.zb.as<float>(), nullptr, 0, wq, HD, nb,
                (int)HD, d, s);
    launch_cls_attn_fold(wq, U, mB, c.mask, nb, S, d, H, zq, s);
    launch_gemm(EPI_BIAS_F16, zq, 2 * HD, L.wv_bd.as<half_t>(), L.dqkv.as<float>() + 2 * d, nullptr,
                0, ctx, d, nb, d, (int)(2 * HD), s);
    return;  // ctx is written: no attention launch
  } else if (last && d % 256 == 0) {  // CLS-only last layer: K, V for all rows, Q for CLS rows
    LnFold lkv = lq;
    lkv.colsum = L.cqkv.as<float>() + d;
    launch_gemm(EPI_LNF_F16, U, d, L.wqkv_f.as<half_t>() + (int64_t)d * d, L.dqkv.as<float>() + d,
                nullptr, 0, qkv + d, 3 * d, M, 2 * d, d, s, &lkv);
    launch_gemm(EPI_LNF_F16, U, (int64_t)S * d, L.wqkv_f.as<half_t>(), L.dqkv.as<float>(), nullptr,
                0, qkv, (int64_t)S * 3 * d, nb, d, d, s, &lc);
  } else {
    launch_gemm(EPI_LNF_F16, U, d, L.wqkv_f.as<half_t>(), L.dqkv.as<float>(), nullptr, 0, qkv,
                3 * d, M, 3 * d, d, s, &lq);
  }
  launch_attention(qkv, c.mask, ctx, nb, S, last ? 1 : S, d, H, s);
}

// O-projection + residual LN2(l-1)(u) -> u1 (in place, or compact rows) + partials sA -> mA
void Encoder::fold_oproj(const Chunk& c, size_t l, bool last) {
  const Layer& L = layers_[l];
  const Layer* P = l > 0 ? &layers_[l - 1] : nullptr;
  const int d = cfg_.hidden, S = c.S;
  const int Mr = last ? c.nb : c.M;
  half_t* Uo = last ? c.Uc : c.U;
  LnFold lo;
  lo.mr = c.mB;
  lo.stat_ld = last ? S : 1;
  lo.gamma = P ? P->ln2g.as<float>() : nullptr;
  lo.stat_out = c.sA;
  lo.y8 = plan_.ffn1 ? c.u8 : nullptr;  // e4m3 copy of u1 for the fp8 FFN1
  const int eo = plan_.ffn1 ? (l == 0 ? EPI_RES16_STATS_Y8 : EPI_LNR16_STATS_Y8)
                            : (l == 0 ? EPI_RES16_STATS : EPI_LNR16_STATS);
  if (c.o8 && !last) {  // e4m3 ctx (K5c) x e4m3 W_o rows on the block-scaled fp8 MFMA
    lo.wexp = L.woe.as<uint8_t>();
    launch_gemm_f8w(eo, c.ctx8, d, L.wo_8.as<uint8_t>(), (l == 0 ? L.bo : L.bo_f).as<float>(), c.U,
                    d, Uo, d, Mr, d, d, c.s, &lo);
  } else {
    launch_gemm(eo, ctx_.as<half_t>(), d, L.wo.as<half_t>(),
                (l == 0 ? L.bo : L.bo_f).as<float>(), c.U, last ? (int64_t)S * d : d, Uo, d, Mr,
                d, d, c.s, &lo);
  }
  launch_ln_stats_finalize(c.sA, d / 128, cfg_.ln_eps, Mr, c.mA, c.s);
}

// FFN1 on LN1(u1) folded; FFN2 + residual LN1(u1) -> u2 (in place) + partials sB -> mB
void Encoder::fold_ffn(const Chunk& c, size_t l, bool last) {
  const Layer& L = layers_[l];
  const int d = cfg_.hidden, F = cfg_.intermediate;
  const int Mr = last ? c.nb : c.M;
  half_t* Uo = last ? c.Uc : c.U;
  half_t* ffn = ffn_.as<half_t>();
  LnFold l1;
  l1.mr = c.mA;
  l1.colsum = L.c1.as<float>();
  if (plan_.ffn1) {
    l1.colsum = L.c1_8.as<float>();
    l1.wexp = L.w1e.as<uint8_t>();
    launch_gemm_f8w(EPI_LNF_GELU_F8, c.u8, d, L.w1_8.as<uint8_t>(), L.d1.as<float>(), nullptr, 0,
                    ffn, F, Mr, F, d, c.s, &l1);
  } else {
    launch_gemm(plan_.ffn2 ? EPI_LNF_GELU_F8 : EPI_LNF_GELU_F16, Uo, d, L.w1_f.as<half_t>(),
                L.d1.as<float>(), nullptr, 0, ffn, F, Mr, F, d, c.s, &l1);
  }
  LnFold l2;
  l2.mr = c.mA;
  l2.gamma = L.ln1g.as<float>();
  l2.stat_out = c.sB;
  l2.wexp = L.w2e.as<uint8_t>();
  l2.y8 = (plan_.qkv && !plan_.qkv_norm && !last) ? c.u8 : nullptr;  // e4m3 copy of u2 for the next fp8 QKV
  if (plan_.ffn2)  // ffn holds e4m3 bytes (F per row)
    launch_gemm_f8w(l2.y8 ? EPI_LNR16_STATS_Y8 : EPI_LNR16_STATS, reinterpret_cast<const uint8_t*>(ffn), F,
                    L.w2_8.as<uint8_t>(), L.b2_f.as<float>(), Uo, d, Uo, d, Mr, d, F, c.s, &l2);
  else
    launch_gemm(EPI_LNR16_STATS, ffn, F, L.w2h.as<half_t>(), L.b2_f.as<float>(), Uo, d, Uo,
                d, Mr, d, F, c.s, &l2);
  launch_ln_stats_finalize(c.sB, d / 128, cfg_.ln_eps, Mr, c.mB, c.s);
  if (plan_.qkv_norm && l + 1 < layers_.size()) launch_quantize_norm_fp8(Uo, d, c.mB, Mr, d, c.u8, c.s);
}

// The layers with materialised LayerNorms (fp32 residual stream, or SR_LN_FOLD=0)
void Encoder::unfolded_stack(const Chunk& c) {
  const int d = cfg_.hidden, F = cfg_.intermediate, H = cfg_.heads, S = c.S, nb = c.nb, M = c.M;
  half_t* h16 = h16_.as<half_t>();
  half_t* qkv = qkv_.as<half_t>();
  half_t* ctx = ctx_.as<half_t>();
  half_t* ffn = ffn_.as<half_t>();
  void* y = y32_.p;  // bias + residual sum: fp32, or fp16 with an fp16 residual stream
  const bool res16 = cfg_.residual_fp16 != 0;
  const void* hres = res16 ? (const void*)h16 : (const void*)h32_.p;  // residual operand
  float* h32w = res16 ? nullptr : h32_.as<float>();
  const int epi_res = res16 ? EPI_BIAS_RES_F16 : EPI_BIAS_RES_F32;
  // split weights: W = [hi | lo] (N x 2K), the GEMM's K is 2K over the repeated activation
  const int kr = split_ ? 2 : 1;
  auto lin = [&](int epi, const half_t* X, int64_t lda, const half_t* W, const float* b,
                 const void* R, int64_t ldr, void* Y, int64_t ldy, int Mm, int Nn, int Kx) {
    LnFold lx;
    lx.x_k = split_ ? Kx : 0;
    lx.chunk_ws = chunk_ws_.as<float>();
    lx.chunk_ws_bytes = (int64_t)chunk_ws_.bytes;
    launch_gemm(epi, X, lda, W, b, R, ldr, Y, ldy, Mm, Nn, kr * Kx, c.s, &lx);
  };
  for (size_t l = 0; l < layers_.size(); ++l) {
    const Layer& L = layers_[l];
    const bool last = c.cls_only && l + 1 == layers_.size();
    lin(EPI_BIAS_F16, h16, d, L.wqkv.as<half_t>(), L.bqkv.as<float>(), nullptr, 0, qkv, 3 * d, M,
        3 * d, d);
    // rows of the rest of the block: all M tokens, or the nb CLS rows (compact) in the last layer
    const int Mr = last ? nb : M;
    launch_attention(qkv, c.mask, ctx, nb, S, last ? 1 : S, d, H, c.s);
    lin(epi_res, ctx, d, L.wo.as<half_t>(), L.bo.as<float>(), hres, last ? (int64_t)S * d : d, y,
        d, Mr, d, d);
    launch_layernorm(y, res16, L.ln1g.as<float>(), L.ln1b.as<float>(), cfg_.ln_eps, Mr, d, h16,
                     h32w, c.s);
    lin(EPI_BIAS_GELU_F16, h16, d, L.w1.as<half_t>(), L.b1.as<float>(), nullptr, 0, ffn, F, Mr, F,
        d);
    lin(epi_res, ffn, F, L.w2.as<half_t>(), L.b2.as<float>(), hres, d, y, d, Mr, d, F);
    launch_layernorm(y, res16, L.ln2g.as<float>(), L.ln2b.as<float>(), cfg_.ln_eps, Mr, d, h16,
                     h32w, c.s);
  }
}

// Pooled embeddings (+ the token heads) or classifier logits of the chunk, from the final states:
// row b*S of each sequence, or row b (compact) after a CLS-only last layer
void Encoder::output_stage(const Chunk& c, int mode, int pool, void* out, int out_dtype, int ld_out,
                           const TokenHeads* heads, float* tok_weight) {
  const int d = cfg_.hidden, S = c.S, nb = c.nb, M = c.M;
  const int64_t b0 = c.b0;
  half_t* h16 = h16_.as<half_t>();
  const bool res16 = cfg_.residual_fp16 != 0;
  const void* hfin = res16 ? (const void*)h16 : (const void*)h32_.p;
  const int Sf = c.cls_only ? 1 : S;
  if (mode == 1) {
    float* t = clst_.as<float>();
    launch_gemm(EPI_BIAS_TANH_F32, h16, (int64_t)Sf * d, wc_.as<half_t>(), bc_.as<float>(),
                nullptr, 0, t, d, nb, d, d, c.s);
    launch_cls_logits(t, wout_.as<float>(), bout_.as<float>(), nb, d, cfg_.num_labels,
                      reinterpret_cast<float*>(out) + b0 * cfg_.num_labels, c.s);
    return;
  }
  const size_t esz = out_dtype == SR_DTYPE_F32 ? sizeof(float) : sizeof(half_t);
  launch_pool_l2(hfin, res16, c.mask, nb, Sf, d, pool,
                 reinterpret_cast<char*>(out) + (size_t)b0 * ld_out * esz, out_dtype, ld_out, c.s);
  if (heads && heads->sparse) {  // this chunk's token weights and terms, at the chunk's offset into B x S
    const SparseOut* sparse = heads->sparse;
    float* tw = tok_weight + b0 * S;
    launch_sparse_token_weights(hfin, res16, c.mask, sparse_w_.as<float>(), sparse_b_.as<float>(), M, d,
                                tw, c.s);
    launch_sparse_terms(c.ids, c.mask, tw, nb, S, sparse->special_ids, sparse->n_special,
                        sparse->terms + b0 * S, sparse->weights + b0 * S, sparse->count + b0, c.s);
  }
  if (heads && heads->multivec) {  // v = W h + b for every token of the chunk (fp16), then normalise and compact
    const MultiVecOut* mv = heads->multivec;
    const int dc = colbert_dc_;
    half_t* v = colbert_v_.as<half_t>();
    launch_gemm(EPI_BIAS_F16, h16, d, colbert_w_.as<half_t>(), colbert_b_.as<float>(), nullptr, 0, v,
                dc, M, dc, d, c.s);
    launch_colbert_pack(v, c.mask, nb, S, dc, mv->vecs + b0 * S * dc, mv->len + b0, c.s);
  }
}

void Encoder::forward_host(const int32_t* ids, const int32_t* mask, const int32_t* types, int B,
                           int S, int mode, int pool, float* out, const SparseOut* sparse,
                           const MultiVecHost* mv) {
  SR_CHECK(B >= 0 && S >= 1, "encoder: bad batch shape");
  SR_CHECK(B == 0 || (ids && mask && out && (!mv || (mv->vecs && mv->len)) &&
                      (!sparse || (sparse->terms && sparse->weights && sparse->count))),
           "encoder: null buffer");
  if (sparse) sparse_terms_check_args(B, S, sparse->n_special);
  if (mv) {  // the head's width sizes the staging
    if (!(colbert_w_set_ && colbert_b_set_))
      throw Error(SR_ERR_STATE, std::string("encoder: weight not set: colbert_linear.") +
                                    (colbert_w_set_ ? "bias" : "weight"));
    colbert_pack_check_args(B, S, colbert_dc_);
  }
  if (B == 0) return;
  DeviceGuard g(device_);
  const size_t n = (size_t)B * S, nv = mv ? n * colbert_dc_ : 0;
  const size_t out_elems = (size_t)B * (mode == 0 ? cfg_.hidden : cfg_.num_labels);
  int32_t *dids, *dmask, *dtypes = nullptr;
  float* dout;
  SparseOut so{};
  MultiVecOut mo{};
  Carve c;
  c.part(n, &dids, &dmask);
  if (types) c.part(n, &dtypes);
  c.part(out_elems, &dout);
  if (sparse) {
    so.special_ids = sparse->special_ids;
    so.n_special = sparse->n_special;
    c.part(n, &so.tok_weight, &so.terms, &so.weights);
    c.part((size_t)B, &so.count);
  }
  if (mv) {
    c.part(nv, &mo.vecs);
    c.part((size_t)B, &mo.len);
  }
  hostio_.carve(c);
  auto up = [&](int32_t* dst, const int32_t* src) {
    SR_HIP(hipMemcpyAsync(dst, src, n * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
  };
  auto down = [&](void* dst, const void* src, size_t bytes) {
    SR_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream_));
  };
  up(dids, ids);
  up(dmask, mask);
  if (types) up(dtypes, types);
  TokenHeads th;
  th.sparse = sparse ? &so : nullptr;
  th.multivec = mv ? &mo : nullptr;
  forward_dev(dids, dmask, dtypes, B, S, mode, pool, dout, SR_DTYPE_F32, cfg_.hidden, stream_,
              sparse || mv ? &th : nullptr);
  std::vector<half_t> hv(nv);  // the multi-vector output is fp16 on the device, fp32 for the caller
  down(out, dout, out_elems * sizeof(float));
  if (mv) {
    down(hv.data(), mo.vecs, nv * sizeof(half_t));
    down(mv->len, mo.len, (size_t)B * sizeof(int32_t));
  }
  if (sparse) {
    if (sparse->tok_weight) down(sparse->tok_weight, so.tok_weight, n * sizeof(float));
    down(sparse->terms, so.terms, n * sizeof(int32_t));
    down(sparse->weights, so.weights, n * sizeof(float));
    down(sparse->count, so.count, (size_t)B * sizeof(int32_t));
  }
  SR_HIP(hipStreamSynchronize(stream_));
  for (size_t i = 0; i < nv; ++i) mv->vecs[i] = (float)hv[i];
}

}  // namespace sr
