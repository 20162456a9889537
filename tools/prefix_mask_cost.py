"""python tools/prefix_mask_cost.py -- cost of the prefix-slot mask when it is on.  Step time (forward + backward, BERT-base, bs 32, S 128, P 36, ragged lengths, padding-free) with a half-masked batch against the
same batch unmasked, alternating; events around 20 steps after 5 warm-up steps, 4 rounds."""
import os, sys, types, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # tools/ -> repository root
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import torch
import params as P
from transformers import BertConfig
from mtvaf_amd import engine
from mtvaf_amd.models.bert_model import TVNetSAModel2
dev = "cuda"
cfg = P.EncCfg(vocab_size=30522, hidden=768, heads=12, inter=3072, layers=12, max_pos=512)
hf = BertConfig(vocab_size=cfg.vocab_size, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
                max_position_embeddings=512, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
args = types.SimpleNamespace(bert_name="bert-base-uncased", bert_config=hf, use_prefix=True, vao=False, noauxloss=True, use_probe=False,
                             n_gpu=1, alpha=0.0, prefix_len=4, prefix_dim=768, device=dev, resnet_root=None, use_152=False)
torch.manual_seed(0)
LABELS = ["O", "B-NEU", "I-NEU", "B-POS", "I-POS", "B-NEG", "I-NEG", "X", "[CLS]", "[SEP]"]
m = TVNetSAModel2(LABELS, None, args).to(dev).train()
B, S, NA = 32, 128, 8
ids, mask, tt, labels = (t.to(dev) for t in P.text_batch(cfg, 3, B, S, lo_id=1000))
g = torch.Generator().manual_seed(1)
feats = torch.randn(B, 3840, 2, 2, generator=g).abs().to(dev)
aux = torch.randn(B, NA, 3840, 2, 2, generator=g).abs().to(dev)
kw = dict(input_ids=ids, attention_mask=mask, token_type_ids=tt, labels=labels, images=feats, aux_imgs=aux)
half = torch.ones(B, 4 * (1 + NA), device=dev)
half[::2] = 0  # every second sentence without any slot
def run(extra, n):
    for _ in range(n):
        m.zero_grad(set_to_none=True)
        m(**kw, **extra).loss.backward()
def timed(extra):
    run(extra, 5)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); run(extra, 20); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / 20
res = {"unmasked": [], "half_masked": []}
for r in range(4):
    res["unmasked"].append(round(timed({}), 3))
    assert engine.LAST_PMASK is None and engine.LAST_PACK is not None
    res["half_masked"].append(round(timed({"prefix_mask": half}), 3))
    assert engine.LAST_PMASK is not None
print("[prefix-mask-cost] ms per fwd+bwd step:", json.dumps(res), flush=True)
