"""Golden vectors for the masked-LM head: runs the REFERENCE's own BertForMaskedLM (models/modeling_bert.py of the reference
checkout, imported through gen_golden's shim -- none of its text is copied) on CPU at the tiny dimensions of the enc_tiny_bert_*
fixtures and records what tests/test_mlm_gpu.py compares with: mlm_tiny.npz (head weights, ids, labels, loss, the logits of the
labelled rows, gradients of the head parameters and of the tied word table) and mlm_state_keys.json (the state_dict keys).

    python tests/golden/gen_mlm_golden.py

The encoder weights are params.encoder_params(TINY_BERT, SEED): the fixture stores the seed, not the tensors."""
from __future__ import annotations

import json
import os

import numpy as np
import torch

import gen_golden as G
import params as P

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 700


def head_params(cfg: P.EncCfg, seed: int):
    g = torch.Generator().manual_seed(seed)
    n = lambda *s, std=0.05: torch.randn(*s, generator=g) * std
    return {"cls.predictions.transform.dense.weight": n(cfg.hidden, cfg.hidden),
            "cls.predictions.transform.dense.bias": n(cfg.hidden),
            "cls.predictions.transform.LayerNorm.weight": 1.0 + n(cfg.hidden),
            "cls.predictions.transform.LayerNorm.bias": n(cfg.hidden),
            "cls.predictions.bias": n(cfg.vocab_size, std=0.2)}


def main():
    G.install_shim()
    from models.modeling_bert import BertForMaskedLM
    cfg = P.TINY_BERT
    B, S = 3, 16
    m = BertForMaskedLM(G.ref_config(cfg))
    keys = sorted(k for k in m.state_dict() if "position_ids" not in k)
    with open(os.path.join(HERE, "mlm_state_keys.json"), "w") as f:
        json.dump({"BertForMaskedLM": keys, "head": [k[len("cls."):] for k in keys if k.startswith("cls.")]}, f, indent=1)
    sde, sdh = P.encoder_params(cfg, SEED), head_params(cfg, SEED + 1)
    sd = {**{"bert." + k: v for k, v in sde.items() if not k.startswith("pooler.")}, **sdh}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    assert all("position_ids" in k or "decoder" in k for k in missing), missing
    m.tie_weights() if hasattr(m, "tie_weights") else None
    m.cls.predictions.decoder.weight = m.bert.embeddings.word_embeddings.weight  # the tie, whatever the shim left of it
    m.train()
    ids, mask, tt, _ = P.text_batch(cfg, SEED + 2, B, S, lengths=[16, 9, 5])
    rng = np.random.default_rng(SEED + 3)
    labels = torch.full((B, S), -100, dtype=torch.long)
    pick = torch.from_numpy(rng.random((B, S)) < 0.3) & mask.bool()
    pick[0, 0] = True
    labels[pick] = ids[pick]
    masked = ids.clone()
    masked[pick] = torch.from_numpy(rng.integers(3, cfg.vocab_size, size=int(pick.sum())))
    out = m(input_ids=masked, attention_mask=mask, token_type_ids=tt, labels=labels, return_dict=True)
    out["loss"].backward()
    named = dict(m.named_parameters())
    fx = {"seed": SEED, "B": B, "S": S, "ids": masked.numpy(), "mask": mask.numpy(), "tt": tt.numpy(), "labels": labels.numpy(),
          "loss": out["loss"].detach().numpy(), "logits_sel": out["logits"].detach()[pick].numpy(),
          "g_word": named["bert.embeddings.word_embeddings.weight"].grad.numpy(),
          "g_q0_w": named["bert.encoder.layer.0.attention.self.query.weight"].grad.numpy()}
    for k, v in sdh.items():
        fx["w:" + k] = v.numpy()
        fx["g:" + k] = named[k].grad.numpy()
    np.savez_compressed(os.path.join(HERE, "mlm_tiny.npz"), **fx)
    print(f"[golden] mlm_tiny: loss {float(out['loss']):.6f}, {int(pick.sum())} labelled rows, "
          f"{os.path.getsize(os.path.join(HERE, 'mlm_tiny.npz'))} bytes")


if __name__ == "__main__":
    main()
