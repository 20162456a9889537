"""BertForMaskedLM on the MI355X against tests/golden/mlm_tiny.npz (the reference's own BertForMaskedLM on CPU): loss, the logits
of the labelled rows, gradients of the head, of an encoder weight and of the tied word table, at the tolerances of
tests/test_oracle_golden.py (outputs rtol 1e-4 / atol 2e-5; gradients rtol 2e-3 / atol 2e-5 max(1, |ref|max)); and the tied table's
gradient against embedding contribution + decoder contribution of an untied copy.  Called by tests/test_mlm_gpu.py in-process and,
as a script, in a child process whose environment sets MTVAF_DIRECT_GRADS=0 (the switch is read when the engine is imported)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (os.path.dirname(HERE), HERE, os.path.join(HERE, "golden")) if p not in sys.path]

DEV = "cuda"


def build(fx, tie=True, chunk=32):
    import params as P
    from test_model_gpu import hf_config
    from mtvaf_amd.models.modeling_bert import BertForMaskedLM
    cfg = P.TINY_BERT
    m = BertForMaskedLM(hf_config(cfg), tie=tie, chunk=chunk)  # V = 64: two chunks
    sd = {"bert." + k: v for k, v in P.encoder_params(cfg, int(fx["seed"])).items() if not k.startswith("pooler.")}
    sd.update({k[2:]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("w:")})
    if not tie:
        sd["cls.predictions.decoder.weight"] = sd["bert.embeddings.word_embeddings.weight"].clone()
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all("position_ids" in k or "decoder" in k for k in missing), (missing, unexpected)
    return m.to(DEV).train()


def grad_close(got, ref, name):
    ref = np.asarray(ref)
    np.testing.assert_allclose(got.detach().cpu().numpy(), ref, rtol=2e-3, atol=2e-5 * max(1.0, float(np.abs(ref).max())), err_msg=name)


def check():
    from mtvaf_amd import engine
    fx = dict(np.load(os.path.join(HERE, "golden", "mlm_tiny.npz")))
    ids, mask, tt, labels = (torch.from_numpy(fx[k]).to(DEV) for k in ("ids", "mask", "tt", "labels"))
    m = build(fx)
    loss, logits = m(input_ids=ids, attention_mask=mask, token_type_ids=tt, labels=labels, output_logits=True)
    loss.backward()
    n = int((labels != -100).sum())
    np.testing.assert_allclose(float(loss.detach()), float(fx["loss"]), rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(logits.detach()[:n].cpu().numpy(), fx["logits_sel"], rtol=1e-4, atol=2e-5)
    assert int(m.cls.last_count) == n
    named = dict(m.named_parameters())
    for k in fx:
        if k.startswith("g:"):
            grad_close(named[k[2:]].grad, fx[k], k)
    grad_close(named["bert.encoder.layer.0.attention.self.query.weight"].grad, fx["g_q0_w"], "g_q0_w")
    g_tied = named["bert.embeddings.word_embeddings.weight"].grad
    grad_close(g_tied, fx["g_word"], "g_word (tied)")
    # the two contributions, from an untied copy of the same weights
    u = build(fx, tie=False)
    u(input_ids=ids, attention_mask=mask, token_type_ids=tt, labels=labels)[0].backward()
    parts = u.bert.embeddings.word_embeddings.weight.grad + u.cls.predictions.decoder.weight.grad
    assert float(u.cls.predictions.decoder.weight.grad.abs().max()) > 0 and float(u.bert.embeddings.word_embeddings.weight.grad.abs().max()) > 0
    err = float((g_tied - parts).abs().max())
    scale = float(parts.abs().max())
    print(f"direct_grads={engine.DIRECT_GRADS}: loss {float(loss.detach()):.6f} (golden {float(fx['loss']):.6f}); tied table gradient "
          f"vs the sum of its parts: max err {err:.3e} at scale {scale:.3e}")
    assert err <= 2.0 ** -22 * scale  # one fp32 add of two fp32 values, in either order
    # a second backward accumulates into .grad (accumulation_steps > 1): exactly twice the gradient
    m(input_ids=ids, attention_mask=mask, token_type_ids=tt, labels=labels)[0].backward()
    assert float((named["bert.embeddings.word_embeddings.weight"].grad - 2 * parts).abs().max()) <= 2.0 ** -20 * scale
    assert float((named["cls.predictions.bias"].grad - 2 * torch.from_numpy(fx["g:cls.predictions.bias"]).to(DEV)).abs().max()) \
        <= 4e-3 * float(np.abs(fx["g:cls.predictions.bias"]).max())


if __name__ == "__main__":
    check()
    print("ok")
