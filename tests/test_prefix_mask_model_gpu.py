"""The per-sentence prefix-slot mask at the public surface: `BertModel` honours masked prefix columns of its
attention_mask on the padding-free run; `TVNetSAModel2` / `TVNetSAModel` take ``prefix_mask`` / ``image_present`` / ``aux_present``
and args.modality_dropout.  Padding-free against padded runs are compared the way tests/test_unpad_gpu.py compares them (loss
2e-6 relative, equal tags, `close` at rtol 2e-5 with an absolute term of 4e-6 of the largest entry for gradients, 1e-4 for the
atomically accumulated word embeddings)."""
import pytest
import torch

import params as P
from mtvaf_amd import engine
from test_model_gpu import DEV, LABELS, _prompt_inputs, close, hf_config, make_args

pytestmark = pytest.mark.gpu

CFG = P.EncCfg(vocab_size=500, hidden=128, heads=2, inter=256, layers=2, max_pos=64)
B, S, N_AUX = 8, 64, 2
PN = 4 * (1 + N_AUX)
LENGTHS = [20, S, 9, 31, 14, 26, 17, 1]  # 182 of 512 rows: the run packs; the longest sentence is not the first


def _slots():
    """bool [B, PN]: sentence 1 without any slot, 2 without its main image, 3 without its second crop, 4 with single holes."""
    m = torch.ones(B, PN, dtype=torch.bool)
    m[1] = False
    m[2, :4] = False
    m[3, 8:] = False
    m[4, [1, 6, 11]] = False
    return m


def _tagger(dropout=0.0, **kw):
    from mtvaf_amd.models.bert_model import TVNetSAModel2
    args = make_args(alpha=0.0, **kw)
    args.bert_config = hf_config(CFG, dropout=dropout)
    torch.manual_seed(7)
    return TVNetSAModel2(LABELS, None, args).to(DEV)


def _batch():
    ids, mask, tt, labels = P.text_batch(CFG, 91, B, S, LENGTHS, lo_id=5)
    feats, aux, _ = _prompt_inputs(92, B, N_AUX)
    return {k: v.to(DEV) for k, v in dict(input_ids=ids, attention_mask=mask, token_type_ids=tt, labels=labels, images=feats,
                                          aux_imgs=aux).items()}


def _step(m, kw, unpad):
    with engine.padding_free(unpad):
        m.zero_grad(set_to_none=True)
        out = m(**kw)
        masked = engine.LAST_PMASK is not None  # (whether the encoder's attention launches carried a slot mask)
        out.loss.backward()
        torch.cuda.synchronize()
        return (float(out.loss.detach()), [list(t) for t in out.logits], {n: p.grad.clone() for n, p in m.named_parameters()
                                                                           if p.grad is not None},
                engine.LAST_PACK is not None, masked)


def _assert_same_step(a, b):
    """test_unpad_gpu.test_unpadded_run_equals_padded_run's comparison of a padded and a padding-free step."""
    assert abs(a[0] - b[0]) <= 2e-6 * abs(a[0]), (a[0], b[0])
    assert a[1] == b[1]
    assert set(a[2]) == set(b[2])
    for n in a[2]:
        if "word_embeddings" in n:
            close(b[2][n], a[2][n], rtol=1e-4, atol=2e-6 * float(a[2][n].abs().max()), name=n)
        else:
            close(b[2][n], a[2][n], rtol=2e-5, atol=4e-6 * float(a[2][n].abs().max()) + 1e-9, name=n)


def test_bert_model_honours_masked_prefix_columns_on_the_padding_free_run():
    """The public seam, with nothing but an attention_mask: zeros in prefix columns change the hidden states of a padding-free
    run exactly as they change those of the padded run."""
    from mtvaf_amd.models.modeling_bert import BertModel
    torch.manual_seed(3)
    bert = BertModel(hf_config(CFG)).to(DEV).eval()
    bert.allow_unpad = True
    ids, mask, tt, _ = (t.to(DEV) for t in P.text_batch(CFG, 91, B, S, LENGTHS, lo_id=5))
    g = torch.Generator().manual_seed(5)
    pkv = torch.randn(CFG.layers, 2, B, PN * CFG.hidden, generator=g).to(DEV)
    full = torch.cat([torch.ones(B, PN, dtype=mask.dtype, device=DEV), mask], 1)
    holes = torch.cat([_slots().to(DEV).to(mask.dtype), mask], 1)
    valid = mask.bool()
    res = {}
    with torch.no_grad():
        for name, am in (("full", full), ("holes", holes)):
            for unpad in (False, True):
                with engine.padding_free(unpad):
                    h = bert(input_ids=ids, attention_mask=am, token_type_ids=tt, past_key_values=pkv).last_hidden_state
                    assert (engine.LAST_PACK is not None) == unpad
                    res[name, unpad] = h.clone()
    close(res["full", True][valid], res["full", False][valid], rtol=2e-5, name="unmasked prefix")
    close(res["holes", True][valid], res["holes", False][valid], rtol=2e-5, name="masked prefix columns")
    # the mask matters (sentences 1 .. 4 lost slots), and only where it was set
    moved = (res["holes", False] - res["full", False]).abs().amax(-1)
    assert float(moved[1:5][valid[1:5]].min()) > 1e-3 and float(moved[[0, 5, 6, 7]].max()) == 0.0


def test_a_direct_encoder_call_does_not_inherit_an_earlier_calls_word():
    """A model call without a mask says "no prefix column is masked" for ITS encoder call only: a later direct
    ``model.bert(..., attention_mask=m)`` with zeros in prefix columns is honoured on the padding-free run whatever ran before."""
    m = _tagger().eval()
    kw = _batch()
    _step(m, kw, True)
    assert m.last_prefix_slots is None and engine.LAST_PMASK is None
    g = torch.Generator().manual_seed(5)
    pkv = torch.randn(CFG.layers, 2, B, PN * CFG.hidden, generator=g).to(DEV)
    am = torch.cat([_slots().to(DEV).to(kw["attention_mask"].dtype), kw["attention_mask"]], 1)
    valid = kw["attention_mask"].bool()
    hs = []
    with torch.no_grad():
        for unpad in (False, True):
            with engine.padding_free(unpad):
                hs.append(m.bert(input_ids=kw["input_ids"], attention_mask=am, token_type_ids=kw["token_type_ids"],
                                 past_key_values=pkv).last_hidden_state.clone())
                assert (engine.LAST_PACK is not None) == unpad and (engine.LAST_PMASK is not None) == unpad
    close(hs[1][valid], hs[0][valid], rtol=2e-5, name="direct encoder call behind an unmasked model call")


def test_arguments_without_a_prefix_are_an_error():
    m = _tagger(use_prefix=False).eval()
    kw = {k: v for k, v in _batch().items() if k not in ("images", "aux_imgs")}
    inf = {k: kw[k] for k in ("input_ids", "attention_mask", "token_type_ids")}
    for extra in (dict(prefix_mask=torch.ones(B, PN, device=DEV)), dict(image_present=torch.ones(B, device=DEV))):
        for fn, args in ((m.forward, kw), (m.predict, inf), (m.predict_nbest, inf), (m.predict_constrained, inf),
                         (m.predict_posteriors, inf)):
            with pytest.raises(ValueError, match="use_prefix"):
                fn(**args, **extra)


def test_tagger_with_a_prefix_mask_padding_free_equals_padded():
    m = _tagger().eval()
    kw = dict(_batch(), prefix_mask=_slots().to(DEV).long())
    a, b = _step(m, kw, False), _step(m, kw, True)
    assert not a[3] and b[3], "the second run did not pack"
    assert not a[4] and b[4]  # (the attention launches carried the mask, and only when packed)
    _assert_same_step(a, b)
    assert torch.equal(m.last_prefix_slots.cpu(), _slots())
    # (the mask matters: the unmasked step has another loss, and launches no masked kernel)
    plain = _step(m, _batch(), True)
    assert not plain[4] and abs(plain[0] - b[0]) > 1e-6 * abs(b[0])


def test_contract_check_passes_with_a_slot_mask():
    """MTVAF_CHECK_CONTRACT (engine.CHECK_CONTRACT): the masked-rows check of the backward runs with a slot mask as without, on the
    packed and on the padded run, and changes nothing."""
    m = _tagger().eval()
    kw = dict(_batch(), prefix_mask=_slots().to(DEV))
    ref = _step(m, kw, True)
    was, engine.CHECK_CONTRACT = engine.CHECK_CONTRACT, True
    try:
        got = _step(m, kw, True)
        _step(m, kw, False)
    finally:
        engine.CHECK_CONTRACT = was
    assert got[3] and got[4] and got[0] == ref[0] and got[1] == ref[1]


def test_no_mask_is_the_all_ones_mask():
    m = _tagger().eval()
    a = _step(m, _batch(), True)
    assert m.last_prefix_slots is None and not a[4]
    b = _step(m, dict(_batch(), prefix_mask=torch.ones(B, PN, device=DEV)), True)
    assert b[4]
    assert a[0] == b[0] and a[1] == b[1]
    for n in a[2]:
        if "word_embeddings" in n:  # (float atomics: the order of the adds is not fixed)
            close(b[2][n], a[2][n], rtol=1e-4, atol=2e-6 * float(a[2][n].abs().max()), name=n)
        else:
            assert torch.equal(a[2][n], b[2][n]), n


def test_image_present_and_aux_present_expand_to_the_documented_slots():
    from mtvaf_amd.models.bert_model import image_slots
    img = torch.tensor([1, 0, 1, 1, 1, 1, 1, 1])
    aux = torch.ones(B, N_AUX, dtype=torch.long)
    aux[2, 0] = 0
    aux[3, 1] = 0
    want = torch.ones(B, PN, dtype=torch.bool)
    want[1, 0:4] = False   # the main image: slots 0..3
    want[2, 4:8] = False   # crop 0: slots 4..7
    want[3, 8:12] = False  # crop 1: slots 8..11
    assert torch.equal(image_slots(B, N_AUX, "cpu", img, aux), want)
    assert torch.equal(image_slots(B, N_AUX, "cpu", None, aux)[:, :4], torch.ones(B, 4, dtype=torch.bool))
    with pytest.raises(ValueError):
        image_slots(B, N_AUX, "cpu", img, torch.ones(B, N_AUX + 1))
    m = _tagger().eval()
    a = _step(m, dict(_batch(), image_present=img.to(DEV), aux_present=aux.to(DEV)), True)
    assert torch.equal(m.last_prefix_slots.cpu(), want)
    b = _step(m, dict(_batch(), prefix_mask=want.to(DEV)), True)
    assert a[0] == b[0] and a[1] == b[1]
    # ... and the two forms compose by AND
    _step(m, dict(_batch(), image_present=img.to(DEV), prefix_mask=_slots().to(DEV)), True)
    assert torch.equal(m.last_prefix_slots.cpu(), _slots() & image_slots(B, N_AUX, "cpu", img, None))
    with pytest.raises(ValueError):
        m(**dict(_batch(), prefix_mask=torch.ones(B, PN + 1, device=DEV)))


def test_modality_dropout():
    none = torch.zeros(B, PN, device=DEV)
    m = _tagger(modality_dropout=1.0).train()
    # (train mode: the head's dropout draws too -- both steps start from the same generator state and dropout offset, and the
    # modality draw has a generator of its own, so that it does not move the head's)
    m.modality_generator = torch.Generator(device=DEV).manual_seed(11)

    def step(kw):
        torch.manual_seed(5)
        engine.RNG.offset = 0
        return _step(m, kw, True)
    a = step(_batch())
    assert not bool(m.last_prefix_slots.any()) and a[4]
    m.args.modality_dropout = 0.0
    b = step(dict(_batch(), prefix_mask=none))
    assert a[0] == b[0] and a[1] == b[1]  # p = 1: every sentence fully masked
    c = step(_batch())                     # p = 0: no mask is created, no masked launch
    assert m.last_prefix_slots is None and not c[4]
    m.args.modality_dropout = 0.5
    drawn = []
    for _ in range(2):
        m.modality_generator = torch.Generator(device=DEV).manual_seed(11)
        _step(m, _batch(), True)
        drawn.append(m.last_prefix_slots.clone())
    assert torch.equal(drawn[0], drawn[1])
    rows = drawn[0].all(1) | ~drawn[0].any(1)
    assert bool(rows.all()) and 0 < int(drawn[0][:, 0].sum()) < B  # whole prefixes, some kept and some dropped
    mask = _slots().to(DEV)   # composes with a caller's mask by AND
    m.modality_generator = torch.Generator(device=DEV).manual_seed(11)
    _step(m, dict(_batch(), prefix_mask=mask), True)
    assert torch.equal(m.last_prefix_slots, drawn[0] & mask)
    m.eval()                   # eval mode never drops
    _step(m, _batch(), True)
    assert m.last_prefix_slots is None


def test_vao_loss_leaves_out_the_sentences_without_an_image():
    """args.vao: a sentence without an image contributes nothing to that image's tag loss and the divisor counts the sentences that
    have it -- the loss equals the loss of the remaining sentences computed alone, at the tolerance of the existing VAO test
    (tests/test_model_gpu.py: `close` at rtol 1e-4); all present has the bits of no mask; no sentence present gives 0."""
    m = _tagger(vao=True, noauxloss=False).eval()
    feats, aux, lab = (t.to(DEV) for t in _prompt_inputs(92, B, N_AUX))
    heads = [m.img_classifier.weight] + [h.weight for h in list(m.aux_img_classifier)[:N_AUX]]

    def run(f, a, l, present):
        m.zero_grad(set_to_none=True)
        _, main, auxl = m.get_visual_prompt(f, a, l, present=present)
        total = main + sum(auxl)
        total.backward()
        torch.cuda.synchronize()
        return [main.detach().clone()] + [x.detach().clone() for x in auxl], [w.grad.clone() for w in heads]
    present = torch.ones(1 + N_AUX, B, device=DEV)
    present[0, 2] = 0      # sentence 2 has no main image
    present[1, [0, 5]] = 0  # sentences 0 and 5 lack crop 0
    got, ggrad = run(feats, aux, lab, present)
    for k in range(1 + N_AUX):
        keep = present[k].bool()
        want, wgrad = run(feats[keep], aux[keep], lab[keep], None)
        close(got[k], want[k], rtol=1e-4, name=f"image-tag loss of image {k}")
        close(ggrad[k], wgrad[k], rtol=1e-4, name=f"classifier gradient of image {k}")
    plain, pgrad = run(feats, aux, lab, None)
    ones, ograd = run(feats, aux, lab, torch.ones(1 + N_AUX, B, device=DEV))
    assert all(torch.equal(x, y) for x, y in zip(plain, ones)) and all(torch.equal(x, y) for x, y in zip(pgrad, ograd))
    none, ngrad = run(feats, aux, lab, torch.zeros(1 + N_AUX, B, device=DEV))
    assert all(float(x) == 0.0 for x in none) and all(float(g.abs().max()) == 0.0 for g in ngrad)
    # through `forward`: image_present reaches the loss, and a step that drops every prefix has no image-tag loss at all
    m.args.alpha = 0.5
    img = torch.ones(B, device=DEV)
    img[2] = 0
    a = _step(m, dict(_batch(), imagelabel=lab), True)
    b = _step(m, dict(_batch(), imagelabel=lab, image_present=img), True)
    assert b[4] and not a[4] and a[0] != b[0] and all(torch.isfinite(g).all() for g in b[2].values())
    m.args.alpha = 0.0
    base = _step(m, dict(_batch(), imagelabel=lab, prefix_mask=torch.zeros(B, PN, device=DEV)), True)[0]
    m.args.alpha = 0.5
    gone = _step(m, dict(_batch(), imagelabel=lab, prefix_mask=torch.zeros(B, PN, device=DEV)), True)[0]
    assert gone == base


def test_predict_and_the_captured_step_honour_the_mask():
    from mtvaf_amd.graph import GraphedTrainStep
    m = _tagger().eval()
    kw = _batch()
    inf = {k: kw[k] for k in ("input_ids", "attention_mask", "token_type_ids")}
    mask = _slots().to(DEV).long()
    with engine.padding_free(False):
        want = m.predict(**inf, images=kw["images"], aux_imgs=kw["aux_imgs"], prefix_mask=mask)
        plain = m.predict(**inf, images=kw["images"], aux_imgs=kw["aux_imgs"])
    got = m.predict(**inf, images=kw["images"], aux_imgs=kw["aux_imgs"], prefix_mask=mask)
    assert engine.LAST_PACK is not None
    assert torch.equal(got["tags"], want["tags"]) and torch.equal(got["count"], want["count"])
    close(got["log_confidence"], want["log_confidence"], rtol=2e-5, name="log_confidence")
    assert not torch.equal(plain["log_confidence"], want["log_confidence"])
    # a captured step runs padded: the mask rides in the static batch
    eager = _step(m, dict(kw, prefix_mask=mask), False)
    m.zero_grad(set_to_none=True)
    step = GraphedTrainStep(m, dict(kw, prefix_mask=torch.ones_like(mask)))
    try:
        out = step(**dict(kw, prefix_mask=mask))
        torch.cuda.synchronize()
        graphed = (float(out.loss), [list(t) for t in out.logits], {n: p.grad.clone() for n, p in m.named_parameters()
                                                                    if p.grad is not None})
        _assert_same_step(eager, graphed)
    finally:
        step.close()


def test_span_model_threads_the_mask():
    from mtvaf_amd.models.bert_model import TVNetSAModel
    M = 5
    args = make_args(use_prefix=True, gcn_layer_number=0, num_layers=0, aug_type="span_cutoff", aug_cutoff_ratio=0.3)
    args.bert_config = hf_config(CFG)
    torch.manual_seed(0)
    m = TVNetSAModel(LABELS, None, args).to(DEV).eval()
    ids, mask, tt, _ = P.text_batch(CFG, 3, B, S, LENGTHS, lo_id=5)
    starts, ends, spos, epos, pol, lm = P.span_batch(CFG, 4, B, S, M, [max(n, 4) for n in LENGTHS])
    feats, aux, _ = _prompt_inputs(11, B, N_AUX)
    kw = {k: v.to(DEV) for k, v in dict(input_ids=ids, attention_mask=mask, token_type_ids=tt, start_positions=spos,
                                        end_positions=epos, span_starts=starts, span_ends=ends, polarity_labels=pol, label_masks=lm,
                                        images=feats, aux_imgs=aux).items()}
    slots = _slots().to(DEV)
    for fn in (m.forward, m.forward_with_cutoff):
        res = []
        for unpad in (False, True):  # (the span model runs padded either way: the argument is threaded, the mask honoured)
            with engine.padding_free(unpad):
                torch.manual_seed(1)
                engine.RNG.offset = 0
                res.append(float(fn(**kw, prefix_mask=slots).loss.detach()))
                assert torch.equal(m.last_prefix_slots, slots)
        torch.manual_seed(1)
        engine.RNG.offset = 0
        plain = float(fn(**kw).loss.detach())
        assert m.last_prefix_slots is None
        assert abs(res[0] - res[1]) <= 2e-6 * abs(res[0]), res
        assert abs(plain - res[0]) > 1e-6 * abs(plain), (plain, res)
    # inference takes the same mask as training: `predict` with it, padding-free setting on and off, and against no mask
    inf = {k: kw[k] for k in ("input_ids", "attention_mask", "token_type_ids", "images", "aux_imgs")}
    with engine.padding_free(False):
        want = m.predict(**inf, prefix_mask=slots)
    got = m.predict(**inf, prefix_mask=slots)
    assert torch.equal(m.last_prefix_slots, slots)
    for k in ("span_starts", "span_ends", "label_masks"):
        assert torch.equal(got[k], want[k]), k
    for k in ("logits", "start_logits", "end_logits", "span_scores"):
        close(got[k], want[k], rtol=2e-5, name=k)
    plain = m.predict(**inf)
    assert m.last_prefix_slots is None and not torch.equal(plain["start_logits"], want["start_logits"])
