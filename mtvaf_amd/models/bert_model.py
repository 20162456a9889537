"""TVNetSAModel2 (CRF tagger, the live model) and TVNetSAModel (span variant) -- the MTVAF task models (BERT/RoBERTa + visual prefix + CRF tagger), MI355X-native.

Drop-in for the reference's ``models/bert_model.py::TVNetSAModel2`` (:416-588): same constructor
``(label_list, tokenizer, args, type_num=None, use_weight=False)``, same ``forward`` signature and
``TokenClassifierOutput(loss, logits=List[List[int]])`` result, same ``get_visual_prompt`` contract and
the same parameter names (``bert.*``, ``fc.*``, ``crf.*``, ``encoder_conv.{0,2}.*``, ``projectors.{i}.*``,
``img_classifier.*``, ``aux_img_classifier.{k}.*``, ``image_model.resnet.*``), so it can be handed to the
reference's ``modules/train.py::SATrainer2`` unchanged.  All arithmetic of the path
runs in the gfx950 kernels behind ``mtvaf_amd.engine``; the sub-modules are parameter containers.

Reference defects the boundary survives: undefined ``args.use_101/use_34/use_18``
flags are read with ``getattr(..., False)``; ``args.n_gpu > 1`` takes the plain loss path (one process
per GPU; the reference's DataParallelCriterion branch, bert_model.py:515-519, cannot run).
"""
from __future__ import annotations

from typing import List, Optional

import torch
from torch import nn
from transformers.modeling_outputs import TokenClassifierOutput

from .. import engine
from ..modules.crf import CRF
from .modeling_bert import BertModel, PrefixKV
from .modeling_roberta import RobertaModel


def _arg(args, name, default=False):
    return getattr(args, name, default)


def _crf_reduction(args):
    """args.crf_reduction: how TVNetSAModel2 reduces the CRF log-likelihood into its loss (the loss stays -llh reduced).
    'mean' (default, the reference's call) | 'token_mean' | 'sum'."""
    reduction = _arg(args, "crf_reduction", "mean")
    if reduction not in ("mean", "token_mean", "sum"):
        raise ValueError(f"args.crf_reduction={reduction!r}: expected 'mean', 'token_mean' or 'sum'")
    return reduction


def _consistency_options(args):
    """The switches of TVNetSAModel2.forward_consistent, checked: args.consistency_weight (0), consistency_ce (True),
    consistency_level ("token" | "chain"), consistency_kind ("sym_kl" | "js"), consistency_temperature (1.0), consistency_aug
    (None | "span_cutoff" | "token_cutoff" | "dim_cutoff")."""
    opt = {"weight": float(_arg(args, "consistency_weight", 0.0) or 0.0), "ce": bool(_arg(args, "consistency_ce", True)),
           "level": _arg(args, "consistency_level", "token"), "kind": _arg(args, "consistency_kind", "sym_kl"),
           "temperature": float(_arg(args, "consistency_temperature", 1.0)), "aug": _arg(args, "consistency_aug", None)}
    for name, allowed in (("level", ("token", "chain")), ("kind", ("sym_kl", "js")),
                          ("aug", (None, "span_cutoff", "token_cutoff", "dim_cutoff"))):
        if opt[name] not in allowed:
            raise ValueError(f"args.consistency_{name}={opt[name]!r}: expected one of {allowed}")
    if not opt["temperature"] > 0:
        raise ValueError(f"args.consistency_temperature={opt['temperature']!r}: expected a positive number")
    return opt


_CHAIN_ONLY = ("crf_risk_weight", "crf_mrt_weight", "crf_entropy_weight")


def _token_head_options(args, num_labels):
    """The switches of the token cross entropy, checked: args.tag_head ("crf" | "softmax"), token_ce_weight
    (0: the auxiliary term beside the CRF), token_ce_reduction ("batch_mean" | "mean" | "sum": the softmax head's loss),
    token_ce_smoothing (0), token_ce_focal_gamma (0, or 1..8), token_ce_class_weights (None | num_labels floats >= 0).  What
    needs a real chain is refused beside the softmax head here, not at the first step."""
    weights = _arg(args, "token_ce_class_weights", None)
    opt = {"head": _arg(args, "tag_head", "crf"), "weight": float(_arg(args, "token_ce_weight", 0.0) or 0.0),
           "reduction": _arg(args, "token_ce_reduction", "batch_mean"), "smoothing": float(_arg(args, "token_ce_smoothing", 0.0) or 0.0),
           "gamma": float(_arg(args, "token_ce_focal_gamma", 0.0) or 0.0),
           "class_weights": None if weights is None else [float(w) for w in weights]}
    if opt["head"] not in ("crf", "softmax"):
        raise ValueError(f"args.tag_head={opt['head']!r}: expected 'crf' or 'softmax'")
    if opt["reduction"] not in ("batch_mean", "mean", "sum"):
        raise ValueError(f"args.token_ce_reduction={opt['reduction']!r}: expected 'batch_mean', 'mean' or 'sum'")
    if opt["weight"] < 0:
        raise ValueError(f"args.token_ce_weight={opt['weight']!r}: expected a number >= 0")
    if not 0.0 <= opt["smoothing"] < 1.0:
        raise ValueError(f"args.token_ce_smoothing={opt['smoothing']!r}: expected a number in [0, 1)")
    if not (opt["gamma"] == 0.0 or 1.0 <= opt["gamma"] <= 8.0):
        raise ValueError(f"args.token_ce_focal_gamma={opt['gamma']!r}: expected 0 or a number in [1, 8]")
    if opt["class_weights"] is not None and (len(opt["class_weights"]) != num_labels or min(opt["class_weights"]) < 0):
        raise ValueError(f"args.token_ce_class_weights: expected {num_labels} weights >= 0 (one per label id, PAD = 0 first), got "
                         f"{weights!r}")
    if opt["head"] == "softmax":
        on = [n for n in _CHAIN_ONLY if _arg(args, n, 0.0)]
        if _arg(args, "crf_reduction", "mean") != "mean":
            on.append("crf_reduction")
        if _arg(args, "consistency_level", "token") == "chain":
            on.append("consistency_level='chain'")
        if on:
            raise ValueError(f"args.tag_head='softmax' has no chain: {', '.join('args.' + n for n in on)} need args.tag_head='crf'")
    return opt


def _entity_scorer(args, label_list):
    """args.score_entities: True (the "seqeval" scheme) or a scheme name -> an `mtvaf_amd.metrics.EntityScorer` over the
    trainer's label map (label_list enumerated from 1, MTVAF_training.py:369); unset / False -> None."""
    want = _arg(args, "score_entities")
    if not want:
        return None
    from ..metrics import EntityScorer
    return EntityScorer({label: i for i, label in enumerate(label_list, 1)}, scheme="seqeval" if want is True else want)


def _calibration_scorer(args, label_list, head):
    """args.score_calibration: "events" (the chunk events of `predict_posteriors`) or "entities" (the entity lists of `predict` /
    `predict_constrained`) -> an `mtvaf_amd.metrics.CalibrationScorer` over the trainer's label map in args.entity_scheme with
    args.calibration_bins (20) bins; unset / False -> None.  The softmax head has no chain, hence no events."""
    want = _arg(args, "score_calibration")
    if not want:
        return None
    if want not in ("events", "entities"):
        raise ValueError(f"args.score_calibration={want!r}: expected 'events' or 'entities'")
    if want == "events" and head == "softmax":
        raise ValueError("args.tag_head='softmax' has no chain: args.score_calibration='events' needs args.tag_head='crf' "
                         "(score 'entities' instead)")
    from ..metrics import CalibrationScorer
    return CalibrationScorer({label: i for i, label in enumerate(label_list, 1)}, scheme=_arg(args, "entity_scheme", "seqeval"),
                             n_bins=int(_arg(args, "calibration_bins", 20) or 20))


def _span_scorer(args):
    """args.score_spans: True (the reference's class names) or a sequence of four class names -> an
    `mtvaf_amd.metrics.SpanScorer` over the span classifier's four outputs; unset / False -> None."""
    want = _arg(args, "score_spans")
    if not want:
        return None
    from ..metrics import SpanScorer
    return SpanScorer() if want is True else SpanScorer(classes=want)


def _layer_mix(args, bert):
    """args.layer_mix (None | "all" | a list of hidden-state indices, 0 = the embedding output) -> a `LayerMix` over the
    encoder's L + 1 hidden states, or None: no module, no parameter, no state-dict key, no launch.
    args.layer_mix_init_last is added to the last chosen state's scalar."""
    spec = _arg(args, "layer_mix", None)
    if spec is None:
        return None
    from ..modules.layer_mix import LayerMix
    return LayerMix(bert.config.num_hidden_layers + 1, spec, _arg(args, "layer_mix_init_last", 0.0) or 0.0)


def _head_state(bert_output, mix):
    """What the heads read: the last hidden state, or -- with a layer mix -- the mixed state."""
    return bert_output["last_hidden_state"] if mix is None else bert_output.mixed_hidden_state


def _mask_word_map(attention_mask, device):
    """The word map without a tokenizer's: every token with ``attention_mask`` 1 is its own word, the others are outside."""
    pos = torch.arange(attention_mask.shape[1], device=device, dtype=torch.int32).expand(attention_mask.shape[0], -1)
    return torch.where(attention_mask.to(device) != 0, pos, torch.full_like(pos, -1))


def _on_second_stream(fn, inputs, join=False):
    """Run the prompt generator (small, low-occupancy GEMMs and mixing kernels) on the engine's second stream so it
    overlaps the embeddings and the first QKV product; the encoder waits for the prefix right before its first
    attention kernel (``PrefixKV.ready_event``).  Autograd runs the generator's backward on the same stream, next to
    the embeddings' backward.  Small batches / CPU tensors / MTVAF_DW_STREAM=0: plain call."""
    ts = [t for t in inputs if isinstance(t, torch.Tensor)]
    if not (engine.DW_SIDE_STREAM and ts and ts[0].is_cuda and ts[0].shape[0] >= 8):  # small batches are host-bound
        return fn()
    main, side = torch.cuda.current_stream(), engine._side_stream(ts[0].device)
    side.wait_stream(main)
    _accumulate_on_producer_stream()
    with torch.cuda.stream(side):
        out = fn()
        ev = torch.cuda.Event()
        ev.record(side)
    for t in ts:
        t.record_stream(side)
    pkv = out[0] if isinstance(out, tuple) else out
    if join or not isinstance(pkv, PrefixKV):
        main.wait_event(ev)
    else:
        pkv.ready_event = ev
    return out


_warned_off = False


def _accumulate_on_producer_stream():
    """The generator's parameter gradients are PRODUCED on the second stream (autograd runs a node's backward on the stream
    its forward ran on), while their AccumulateGrad nodes were created on the default stream when the parameters were: torch
    (>= 2.9) warns about that mismatch on every backward pass.  It is intended here, and it costs no host synchronisation --
    the engine orders the accumulation behind the producer with a stream-to-stream event wait, and the encoder backward
    joins the two streams anyway -- so the warning is switched off once."""
    global _warned_off
    if not _warned_off:
        _warned_off = True
        fn = getattr(torch.autograd.graph, "set_warn_on_accumulate_grad_stream_mismatch", None)
        if fn is not None:
            fn(False)


SLOTS_PER_IMAGE = 4  # prefix slots one image contributes (`_region_features`): slots 0..3 the main image, then 4 per crop


def image_slots(batch, n_aux, device, image_present=None, aux_present=None):
    """``image_present`` [B] / ``aux_present`` [B, n_aux] (non-zero = the sentence has that image; None = all have it) expanded to
    prefix slots: -> bool [B, 4 * (1 + n_aux)], slots 0..3 the main image's, each following group of 4 one crop's."""
    main = torch.ones(batch, 1, dtype=torch.bool, device=device) if image_present is None \
        else image_present.to(device).reshape(batch, 1) != 0
    aux = torch.ones(batch, n_aux, dtype=torch.bool, device=device) if aux_present is None \
        else aux_present.to(device).reshape(batch, -1) != 0
    if aux.shape[1] != n_aux:
        raise ValueError(f"aux_present covers {aux.shape[1]} crops, the prompt was built from {n_aux}")
    return torch.cat([main, aux], dim=1).repeat_interleave(SLOTS_PER_IMAGE, dim=1)


def _prefix_slots(model, B, n_slots, dev, prefix_mask=None, image_present=None, aux_present=None):
    """Which sentence owns which of the prompt's ``n_slots`` slots -- THE place where a model decides it: -> bool
    [B, P], or None when every sentence owns them all.  ``prefix_mask`` [B, P] (non-zero = slot present), ``image_present`` /
    ``aux_present`` (`image_slots`) and, in training mode, args.modality_dropout = p (each sentence loses its whole prefix with
    probability p: one ``torch.rand(B)`` on the device under ``model.modality_generator``, no host sync, capturable) compose by
    AND.  None of them: None, and no tensor is created.  The decision is kept in ``model.last_prefix_slots``; the caller hands
    ``prefix_masked = (slots is not None)`` to the encoder with the mask it builds from it."""
    slots = None
    if prefix_mask is not None:
        if tuple(prefix_mask.shape) != (B, n_slots):
            raise ValueError(f"prefix_mask is {tuple(prefix_mask.shape)}, the prompt has {n_slots} slots for {B} sentences")
        slots = prefix_mask.to(dev) != 0
    if image_present is not None or aux_present is not None:
        img = image_slots(B, n_slots // SLOTS_PER_IMAGE - 1, dev, image_present, aux_present)
        slots = img if slots is None else slots & img
    p = float(_arg(model.args, "modality_dropout", 0.0) or 0.0)
    if p > 0 and model.training:
        keep = torch.rand(B, device=dev, generator=getattr(model, "modality_generator", None)) >= p
        slots = keep[:, None].expand(B, n_slots) if slots is None else slots & keep[:, None]
    model.last_prefix_slots = slots
    return slots


def _no_prefix(model, prefix_mask, image_present, aux_present):
    """A model without ``use_prefix`` has no slots to mask: the arguments are an error, not ignored."""
    if prefix_mask is not None or image_present is not None or aux_present is not None:
        raise ValueError("prefix_mask / image_present / aux_present need args.use_prefix: this model has no visual prefix")
    model.last_prefix_slots = None


def _prompt_attention_mask(model, attention_mask, n_slots, prefix_mask=None, image_present=None, aux_present=None, slots=False):
    """The attention mask extended over the prompt's ``n_slots`` slots: ones, or the slots `_prefix_slots` decides on (``slots``:
    a decision made earlier in the same call, None included)."""
    B, dev = attention_mask.size(0), attention_mask.device
    if slots is False:
        slots = _prefix_slots(model, B, n_slots, dev, prefix_mask, image_present, aux_present)
    prefix = torch.ones((B, n_slots), device=dev, dtype=attention_mask.dtype) if slots is None else slots.to(attention_mask.dtype)
    return torch.cat((prefix, attention_mask), dim=1)


class ImageModel(nn.Module):
    """Frozen ResNet pyramid front-end (reference: models/bert_model.py:63-111).  It is UPSTREAM of the
    accelerated path and runs in plain torch (MIOpen convolutions) on the trunks of
    ``mtvaf_amd/models/resnet.py`` (torchvision's architecture and state_dict names; torchvision itself is not
    required).  ``resnet_root`` holds the reference's ``resnetNN.pth`` files; ``resnet_root="random"`` skips the
    load (synthetic runs).  Pre-extracted region features bypass it (``TVNetSAModel2.get_visual_prompt``,
    ``mtvaf_amd.features``)."""

    def __init__(self, use_152=False, use_101=False, use_34=False, use_18=False, resnet_root=None):
        super().__init__()
        from .resnet import resnet18, resnet34, resnet50, resnet101, resnet152
        name, ctor = (("resnet152", resnet152) if use_152 else ("resnet101", resnet101) if use_101 else
                      ("resnet34", resnet34) if use_34 else ("resnet18", resnet18) if use_18 else ("resnet50", resnet50))
        self.resnet = ctor()
        if resnet_root is not None and resnet_root != "random":
            self.resnet.load_state_dict(torch.load(f"{resnet_root}/{name}.pth", map_location="cpu"))

    def forward(self, x, aux_imgs=None):
        prefix_guids = self.get_resnet_prompt(x)
        if aux_imgs is not None:
            aux_imgs = aux_imgs.permute([1, 0, 2, 3, 4])
            return prefix_guids, [self.get_resnet_prompt(aux_imgs[i]) for i in range(len(aux_imgs))]
        return prefix_guids, None

    def get_resnet_prompt(self, x):
        out = []
        for name, layer in self.resnet.named_children():
            if name in ("fc", "avgpool"):
                continue
            x = layer(x)
            if "layer" in name:
                kernel = x.size(2) // 2
                out.append(nn.functional.avg_pool2d(x, kernel_size=(kernel, kernel), stride=kernel))
        return out


class _PackedLinears:
    """Views the weights of a ModuleList of equal nn.Linear(in, out) as one [n*out, in] operand."""

    def __init__(self, mods: nn.ModuleList):
        n, out, inn = len(mods), mods[0].out_features, mods[0].in_features
        dev = mods[0].weight.device
        self.w = torch.empty(n * out, inn, device=dev)
        self.b = torch.empty(n * out, device=dev)
        with torch.no_grad():
            for i, m in enumerate(mods):
                self.w[i * out:(i + 1) * out].copy_(m.weight.data)
                self.b[i * out:(i + 1) * out].copy_(m.bias.data)
                m.weight.data = self.w[i * out:(i + 1) * out]
                m.bias.data = self.b[i * out:(i + 1) * out]
        self.ptrs = [m.weight.data_ptr() for m in mods] + [m.bias.data_ptr() for m in mods]

    def valid(self, mods) -> bool:
        return self.ptrs == [m.weight.data_ptr() for m in mods] + [m.bias.data_ptr() for m in mods]


def _mlm_options(args, config, tokenizer):
    """The masked-LM switches, checked: args.mlm_head, args.mlm_weight (>= 0; > 0 implies the head),
    args.mlm_probability (0.15), args.mlm_tie (True), args.mlm_chunk (None: the engine's default), args.mlm_mask_token_id and
    args.mlm_special_ids -- from the tokenizer when there is one, else the ids of the bert / roberta base vocabularies."""
    weight = float(_arg(args, "mlm_weight", 0.0) or 0.0)
    if weight < 0:
        raise ValueError(f"args.mlm_weight={weight!r}: expected a number >= 0")
    opt = {"head": bool(_arg(args, "mlm_head", False)) or weight > 0, "weight": weight,
           "probability": float(_arg(args, "mlm_probability", 0.15)), "tie": bool(_arg(args, "mlm_tie", True)),
           "chunk": _arg(args, "mlm_chunk", None), "mask_token_id": None, "special_ids": ()}
    if not opt["head"]:
        return opt
    if not 0.0 < opt["probability"] <= 1.0:
        raise ValueError(f"args.mlm_probability={opt['probability']!r}: expected a number in (0, 1]")
    roberta = "roberta" in args.bert_name
    mask_id, special = _arg(args, "mlm_mask_token_id", None), _arg(args, "mlm_special_ids", None)
    if mask_id is None:
        mask_id = getattr(tokenizer, "mask_token_id", None)
    if mask_id is None:
        mask_id = 50264 if roberta else 103
    if special is None:
        special = getattr(tokenizer, "all_special_ids", None)
    if special is None:
        special = (0, 1, 2, 3, 50264) if roberta else (0, 100, 101, 102, 103)
    special = tuple(sorted({int(i) for i in special}))
    if not 0 <= int(mask_id) < config.vocab_size:
        raise ValueError(f"masked-LM: mask token id {mask_id} is outside the vocabulary of {config.vocab_size} "
                         "(args.mlm_mask_token_id)")
    if len(special) > 8:
        raise ValueError(f"masked-LM: {len(special)} special ids, the kernel takes 8 (args.mlm_special_ids)")
    opt["mask_token_id"], opt["special_ids"] = int(mask_id), special
    return opt


class TVNetSAModel2(nn.Module):
    def __init__(self, label_list, tokenizer, args, type_num=None, use_weight=False):
        super().__init__()
        self.args = args
        self.type_num = type_num
        self.tokenizer = tokenizer
        self.prefix_dim = _arg(args, "prefix_dim", 768)
        self.prefix_len = _arg(args, "prefix_len", 4)

        enc_cls = RobertaModel if "roberta" in args.bert_name else BertModel
        bert_config = _arg(args, "bert_config", None)  # extension: explicit config => random-init encoder
        if bert_config is not None:
            self.bert = enc_cls(bert_config)
        else:
            self.bert = enc_cls.from_pretrained(args.bert_name)
        self.bert.skip_pooler = True  # pooler_output is unused on this path
        # this head reads hidden states through the mask only (fc -> CRF with mask=attention_mask): padding-free execution
        # (engine.UNPAD) may leave zeros at masked positions.  TVNetSAModel's position softmax reads every position: no flag.
        self.bert.allow_unpad = True
        self.last_prefix_mass = None  # [L,B,NH,S] after a forward with args.output_prefix_mass
        self.last_prefix_slots = None  # bool [B,P] after a call that masked prefix slots (None: every sentence owned them all)
        self.modality_generator = None  # torch.Generator of the args.modality_dropout draws (None: the device's default)
        self.last_tag_marginals = None  # [B,S,num_labels] after a forward with args.output_tag_marginals
        self.last_crf_risk = None  # detached device scalar after a forward with labels and args.crf_risk_weight > 0
        self.last_crf_entropy = None  # detached device scalar after a forward with a loss and args.crf_entropy_weight != 0
        self.last_crf_mrt = None  # detached device scalar after a forward with labels and args.crf_mrt_weight > 0
        self.last_word_index = None  # mtvaf_amd.words.WordIndex of the last call that ran on the word axis (args.word_pooling)
        self.layer_mix = _layer_mix(args, self.bert)  # args.layer_mix: the head reads a learned mix of the hidden states
        if _arg(args, "word_pooling", None) not in (None, "first", "last", "mean"):
            raise ValueError(f"args.word_pooling={args.word_pooling!r}: expected None, 'first', 'last' or 'mean'")
        hidden = self.bert.config.hidden_size
        self.num_labels = len(label_list) + 1

        if _arg(args, "use_prefix"):
            small = _arg(args, "use_34") or _arg(args, "use_18")
            self.feat_dim = 960 if small else 3840
            if _arg(args, "resnet_root", None) is not None:
                self.image_model = ImageModel(use_152=_arg(args, "use_152"), use_101=_arg(args, "use_101"),
                                              use_34=_arg(args, "use_34"), use_18=_arg(args, "use_18"),
                                              resnet_root=args.resnet_root)
            else:
                self.image_model = None  # region features are fed directly (synthetic / cached features)
            self.encoder_conv = nn.Sequential(nn.Linear(self.feat_dim, 800), nn.Tanh(), nn.Linear(800, 4 * 2 * hidden))
            n_layers = self.bert.config.num_hidden_layers
            self.projectors = nn.ModuleList([nn.Linear(4 * hidden * 2, 4) for _ in range(n_layers)])
            self.img_dropout = nn.Dropout(0.2)
            self.img_classifier = nn.Linear(4 * 2 * hidden, 2089)
            self.aux_img_classifier = nn.ModuleList([nn.Linear(4 * 2 * hidden, 2089) for _ in range(3)])
            self._packed_proj: Optional[_PackedLinears] = None

        # args.tag_head = "softmax": no trainable chain -- the loss is the token cross entropy, the tags are per-token maxima, and
        # self.crf is a chain of zero buffers for the code that reports posteriors (`predict`); args.token_ce_weight > 0 adds the
        # same cross entropy beside the CRF's loss.  Without either nothing is built and nothing is launched.
        self.token_opt = _token_head_options(args, self.num_labels)
        self.token_ce = None
        self.last_token_ce = None  # detached device scalar after a forward with labels and args.token_ce_weight > 0
        if self.token_opt["head"] == "softmax" or self.token_opt["weight"] > 0:
            from ..modules.token_head import TokenCrossEntropy
            self.token_ce = TokenCrossEntropy(self.num_labels, self.token_opt["class_weights"], self.token_opt["smoothing"],
                                              self.token_opt["gamma"])
        if self.token_opt["head"] == "softmax":
            from ..modules.token_head import zero_chain
            self.crf = zero_chain(self.num_labels)
        else:
            self.crf = CRF(self.num_labels, batch_first=True)
        self.fc = nn.Linear(hidden, self.num_labels)
        self.dropout = nn.Dropout(0.1)
        _crf_reduction(args)  # (a misspelt reduction is an error here, not at the first step)
        _consistency_options(args)  # (the same for the switches of forward_consistent)
        # args.score_entities: every forward with labels adds its entity counts to model.entity_scorer on the device (one small
        # launch behind the Viterbi kernel, on its tags); without the switch nothing is launched
        self.entity_scorer = _entity_scorer(args, label_list)
        # args.score_calibration: `predict_posteriors` ("events") or `predict` / `predict_constrained` ("entities") with labels
        # add their batch to model.calibration_scorer on the device; without the switch, or without labels, nothing is launched
        self.calibration_scorer = _calibration_scorer(args, label_list, self.token_opt["head"])
        self.label_list = list(label_list)
        self._predict_tables = None  # (device, scheme) -> the scheme tables of `predict`, built at its first call
        if _arg(args, "use_probe"):
            raise NotImplementedError("the structural probe (probes/) is off the hot path and its import chain is "
                                      "broken in the reference (models/bert_model.py:468-475)")
        # args.mlm_head (or args.mlm_weight > 0): a masked-LM head on the encoder, its decoder tied to the word table (DESIGN.md
        # section 4.32) -- `forward_mlm`, and with the weight an auxiliary term of `forward`.  Without either nothing is built.
        self.mlm_opt = _mlm_options(args, self.bert.config, tokenizer)
        self.last_mlm_loss = None  # detached device scalar after a forward with labels and args.mlm_weight > 0
        self.last_mlm_stats = None  # int32 [3] on the device after a masking call: eligible, selected, dropped for capacity
        if self.mlm_opt["head"]:
            from ..modules.mlm_head import MaskedLMHead
            self.mlm_head = MaskedLMHead(self.bert.config, self.bert.get_input_embeddings(),
                                         style="roberta" if "roberta" in args.bert_name else "bert", tie=self.mlm_opt["tie"],
                                         chunk=self.mlm_opt["chunk"])

    # ------------------------------------------------------------------------------------------------
    def _mlm_pass(self, input_ids, attention_mask, token_type_ids, prefix_guids, prompt_attention_mask, probability=None):
        """Masks on the device and runs the encoder on the masked ids under the given prompt -> the MLM loss (mean over the
        selected tokens).  The selected positions are attended tokens, so the padding-free run holds their hidden rows."""
        from .. import mlm
        opt = self.mlm_opt
        if not opt["head"]:
            raise ValueError("this model was built without args.mlm_head")
        picked = mlm.mask_tokens(input_ids, attention_mask, mask_token_id=opt["mask_token_id"], vocab_size=self.bert.config.vocab_size,
                                 special_ids=opt["special_ids"], probability=opt["probability"] if probability is None else probability)
        was = self.bert.encoder.output_prefix_mass
        self.bert.encoder.output_prefix_mass = False
        out = self.bert(input_ids=picked["input_ids"], attention_mask=prompt_attention_mask, token_type_ids=token_type_ids,
                        past_key_values=prefix_guids, return_dict=True, prefix_masked=self.last_prefix_slots is not None)
        self.bert.encoder.output_prefix_mass = was
        self.last_mlm_stats = picked["stats"]
        return self.mlm_head(out.last_hidden_state, picked["positions"], picked["labels"], picked["count"])

    def forward_mlm(self, input_ids=None, attention_mask=None, token_type_ids=None, images=None, aux_imgs=None, prefix_mask=None,
                    image_present=None, aux_present=None, mlm_probability=None):
        """Masked-LM conditioned on the image prefix (args.mlm_head): the visual prompt is computed once,
        tokens are chosen and corrupted on the device (`mtvaf_amd.mlm.mask_tokens`: args.mlm_probability 0.15, the dropout
        generator), the encoder runs on the masked ids and the head returns the mean cross entropy of the chosen tokens.  No image
        labels: the VAO losses are not formed.  ``self.mlm_head.last_accuracy`` / ``last_count`` stay on the device."""
        prefix_guids, _, prompt_attention_mask = self._prompt_prologue(input_ids, attention_mask, None, images, aux_imgs, prefix_mask,
                                                                       image_present, aux_present, vao=False)
        return self._mlm_pass(input_ids, attention_mask, token_type_ids, prefix_guids, prompt_attention_mask, mlm_probability)

    def forward(self, input_ids=None, attention_mask=None, token_type_ids=None, labels=None, imagelabel=None,
                images=None, aux_imgs=None, allowed_tags=None, token_to_word=None, prefix_mask=None, image_present=None, aux_present=None):
        """reference: models/bert_model.py:480-532.  ``prefix_mask`` [B, P] (1 = the sentence owns that visual slot), or its
        convenience form ``image_present`` [B] / ``aux_present`` [B, n_aux] (`image_slots`): a sentence without an image, or with
        fewer crops, does not attend to those slots (args.modality_dropout drops whole prefixes in training).  None:
        every sentence owns every slot, as always.  ``allowed_tags`` int64 [B,S] (`mtvaf_amd.constraints`: per-column tag sets of a
        partly annotated batch), given with ``labels=None``: the loss is ``-CRF.partial_llh`` -- the marginal likelihood of the
        paths the sets permit -- with args.crf_reduction, plus the same ``alpha * img_tag_loss`` term.  Without it the method runs
        the code it always ran.
        args.word_pooling ("first" | "last" | "mean") with ``token_to_word`` int32 [B,S] (`mtvaf_amd.spans.batch_token_to_word`): the
        head runs over WORDS (`mtvaf_amd.words`) -- last_hidden_state is pooled onto the word axis [B,W,H]
        (W = args.max_words or S), and dropout, fc, decoding, the scorer, the marginals and every loss term run there with the
        index' word_mask; ``labels`` / ``allowed_tags`` arrive piece-level and are taken at every word's first piece; ``logits``
        are the tags of the word columns and ``self.last_word_index`` keeps the index.  Without args.word_pooling the map is not
        read and the method runs the code it always ran.
        args.tag_head = "softmax" (DESIGN.md 4.28): the loss is the token cross entropy of the emissions (args.token_ce_reduction,
        default "batch_mean"; args.token_ce_smoothing / _focal_gamma / _class_weights) plus the same ``alpha * img_tag_loss``, and
        ``logits`` are the per-token first maxima (mtvaf_token_argmax); ``allowed_tags`` raises.  args.token_ce_weight > 0 with
        the CRF head adds ``weight * CE(batch_mean)`` of the same emissions; ``self.last_token_ce`` keeps the unweighted value."""
        self._chain_only(allowed_tags is not None, "allowed_tags")
        word_mode = self._word_mode(token_to_word)
        text_mask = attention_mask  # (the word axis replaces attention_mask below; the MLM term masks pieces)
        prefix_guids, img_tag_loss, prompt_attention_mask = self._prompt_prologue(input_ids, attention_mask, imagelabel, images,
                                                                                  aux_imgs, prefix_mask, image_present, aux_present)
        # The attention maps are made on request only (the reference hard-codes output_attentions=True, bert_model.py:496-502, and
        # never reads them): args.output_attentions (True or layer indices) fills TokenClassifierOutput.attentions,
        # args.output_prefix_mass fills self.last_prefix_mass [L,B,NH,S] -- each token's attention on the visual slots --
        # without the full maps.  Without the switches the step launches nothing for them.
        self.bert.encoder.output_prefix_mass = bool(_arg(self.args, "output_prefix_mass"))
        bert_output = self.bert(input_ids=input_ids, attention_mask=prompt_attention_mask,
                                token_type_ids=token_type_ids, past_key_values=prefix_guids,
                                output_attentions=_arg(self.args, "output_attentions"), output_hidden_states=True,
                                return_dict=True, layer_mix=self.layer_mix, prefix_masked=self.last_prefix_slots is not None)
        self.last_prefix_mass = self.bert.encoder.last_prefix_mass if self.bert.encoder.output_prefix_mass else None
        hidden = _head_state(bert_output, self.layer_mix)
        index = None
        if word_mode is not None:
            index, attention_mask, labels, allowed_tags = self._word_targets(attention_mask, token_to_word, labels, allowed_tags)
        emissions = self._emissions(hidden, index, word_mode)
        mask_u8 = attention_mask.to(torch.uint8)
        logits, decoded = self._decode(emissions, mask_u8, labels)
        # args.output_tag_marginals fills self.last_tag_marginals [B,S,num_labels] -- posterior tag probabilities, zeros on
        # padding -- from the marginals kernels; without the switch the step launches nothing for them.
        self.last_tag_marginals = self.crf.marginals(emissions.detach(), mask_u8) \
            if _arg(self.args, "output_tag_marginals") else None
        loss = None
        if labels is not None or allowed_tags is not None:
            loss = self._crf_nll(emissions, mask_u8, labels, allowed_tags)
            extra = _arg(self.args, "alpha", 0.0) * img_tag_loss
            if torch.is_tensor(extra) or extra != 0:  # (adding the literal 0.0 of a VAO-less run is two kernels for nothing)
                loss = loss + extra
        loss = self._posterior_terms(loss, emissions, mask_u8, labels, logits, decoded)
        self.last_mlm_loss = None
        if self.mlm_opt["weight"] > 0 and labels is not None:
            # args.mlm_weight > 0 adds weight * the masked-LM loss of a second pass over the masked ids, under the prompt of the
            # first; self.last_mlm_loss keeps the unweighted value.  At the default 0 the step launches nothing for it.
            if _arg(self.args, "fused_accumulation") and torch.is_grad_enabled():
                self.bert.encoder.grad_sink.begin_two_node_pass()  # (two encoder nodes under one backward, as forward_consistent)
            mlm_loss = self._mlm_pass(input_ids, text_mask, token_type_ids, prefix_guids, prompt_attention_mask)
            self.last_mlm_loss = mlm_loss.detach()
            loss = loss + self.mlm_opt["weight"] * mlm_loss
        if decoded is not None:
            # the decode reads the CRF parameters: whatever follows on the main stream (optimizer.step() updates them in
            # place) is ordered behind it here, not only by the join inside the encoder backward (frozen encoders skip it)
            torch.cuda.current_stream().wait_event(decoded)
        return TokenClassifierOutput(loss=loss, logits=logits, attentions=bert_output.attentions)

    # ---- the pieces of `forward`, shared with `forward_consistent` -----------------------------------------------------
    def _prompt_prologue(self, input_ids, attention_mask, imagelabel, images, aux_imgs, prefix_mask=None, image_present=None,
                         aux_present=None, vao=None):
        """-> (prefix_guids, img_tag_loss, prompt_attention_mask): the visual prompt, its VAO loss (args.vao; else 0) and the attention
        mask extended over the prompt's slots (`_prompt_attention_mask`: the per-sentence slot mask enters here and nowhere else);
        (None, 0, attention_mask) without ``use_prefix``.  ``vao=False``: the VAO losses are left out whatever args.vao says (a
        call without image labels: `forward_mlm`)."""
        vao = _arg(self.args, "vao") if vao is None else vao
        if not _arg(self.args, "use_prefix"):
            _no_prefix(self, prefix_mask, image_present, aux_present)
            return None, 0, attention_mask
        # the slots are decided BEFORE the prompt is generated: the VAO losses leave out the images a sentence does not have
        B, dev = input_ids.size(0), attention_mask.device
        n_img = 1 + (0 if aux_imgs is None else aux_imgs.shape[1])
        slots = _prefix_slots(self, B, SLOTS_PER_IMAGE * n_img, dev, prefix_mask, image_present, aux_present)
        present = None
        if slots is not None and vao:  # [images, B]: a sentence has an image while it owns one of its slots
            present = slots.view(B, n_img, SLOTS_PER_IMAGE).any(-1).t().to(torch.float32).contiguous()
        prefix_guids, img_tag_loss, aux_img_tag_loss = _on_second_stream(
            lambda: self.get_visual_prompt(images, aux_imgs, imagelabel, vao=bool(vao), present=present),
            (images, aux_imgs, imagelabel, present), join=vao)  # the VAO losses are consumed on the main stream right away
        img_tag_loss = img_tag_loss if _arg(self.args, "noauxloss") else img_tag_loss + sum(aux_img_tag_loss)
        if prefix_guids[0][0].shape[2] != SLOTS_PER_IMAGE * n_img:
            raise ValueError(f"the prompt has {prefix_guids[0][0].shape[2]} slots, {n_img} images were expected to give "
                             f"{SLOTS_PER_IMAGE * n_img}")
        return prefix_guids, img_tag_loss, _prompt_attention_mask(self, attention_mask, SLOTS_PER_IMAGE * n_img, slots=slots)

    def _word_targets(self, attention_mask, token_to_word, labels, allowed_tags):
        """The word axis: one launch builds the index; from here on the mask, the labels and the constraint sets are those of the
        word columns.  -> (index, word mask, word labels, word constraint sets)"""
        from ..words import build_word_index, word_allowed, word_labels
        index = build_word_index(attention_mask, token_to_word, _arg(self.args, "max_words", None))
        self.last_word_index = index
        return (index, index.word_mask, None if labels is None else word_labels(labels, index),
                None if allowed_tags is None else word_allowed(allowed_tags, index))

    def _emissions(self, hidden, index, word_mode):
        """The head of one pass: [pool onto the word axis (one launch; fp32, the dtype fc reads in every compute mode) ->] dropout
        -> fc."""
        if index is not None:
            hidden = engine.WordPoolFunction.apply(hidden, index, word_mode)
        sequence_output = engine.dropout(hidden, self.dropout.p, self.training)
        return engine.LinearFunction.apply(sequence_output, self.fc.weight, self.fc.bias, False)

    def _decode(self, emissions, mask_u8, labels):
        """Viterbi paths: device kernel + async packed copy; the list materialises on first use (no mid-step sync).
        One wavefront per sentence is all the parallelism Viterbi and the CRF forward algorithm have, so the two
        run side by side (second stream) instead of back to back.  -> (paths, the event behind them on the second stream or None)
        args.tag_head = "softmax": the per-token maxima in the same packed form, on the main stream (one row launch)."""
        if self.token_opt["head"] == "softmax":
            logits = self.crf.defer_packed(*self._token_tags(emissions.detach(), mask_u8))
            if self.entity_scorer is not None and labels is not None:
                self.entity_scorer.update(logits.device_tags, labels, mask_u8)
            return logits, None
        if emissions.is_cuda and engine.DW_SIDE_STREAM and emissions.shape[0] * emissions.shape[1] >= 1024:  # host-bound below
            main, side = torch.cuda.current_stream(), engine._side_stream(emissions.device)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                logits = self.crf.decode_deferred(emissions.detach(), mask_u8)
                if self.entity_scorer is not None and labels is not None:
                    self.entity_scorer.update(logits.device_tags, labels, mask_u8)
                    labels.record_stream(side)
                decoded = torch.cuda.Event()
                decoded.record(side)
            emissions.record_stream(side)
            mask_u8.record_stream(side)
            return logits, decoded
        logits = self.crf.decode_deferred(emissions, mask_u8)
        if self.entity_scorer is not None and labels is not None:
            self.entity_scorer.update(logits.device_tags, labels, mask_u8)
        return logits, None

    def _token_tags(self, emissions, mask_u8):
        """The softmax head's tags in `CRF.decode_packed`'s form -> (tags int32 [B,S], -1 on masked columns; lengths int32 [B])"""
        tags, _ = self.token_ce.decode(emissions, mask_u8)
        return (torch.where(mask_u8 != 0, tags, torch.full_like(tags, -1)).to(torch.int32),
                mask_u8.sum(dim=1, dtype=torch.int32))

    def _chain_only(self, asked, what):
        if asked and self.token_opt["head"] == "softmax":
            raise ValueError(f"args.tag_head='softmax' has no chain: {what} needs args.tag_head='crf'")

    def _crf_nll(self, emissions, mask_u8, labels, allowed_tags):
        """-llh of the labels, or without them of the paths ``allowed_tags`` permit (`CRF.partial_llh`), under args.crf_reduction.
        args.tag_head = "softmax": the token cross entropy of the labels under args.token_ce_reduction."""
        if self.token_opt["head"] == "softmax":
            return self.token_ce(emissions, labels, mask_u8, self.token_opt["reduction"])
        reduction = _crf_reduction(self.args)
        if labels is None:
            return -self.crf.partial_llh(emissions, allowed_tags, mask=mask_u8, reduction=reduction)
        if reduction == "mean":
            return self.crf.nll_mean(emissions, labels, mask=mask_u8)  # = -1 * crf(..., reduction='mean'), bert_model.py:521
        return -self.crf(emissions, labels, mask=mask_u8, reduction=reduction)

    def _posterior_terms(self, loss, emissions, mask_u8, labels, logits, decoded):
        """``loss`` plus the weighted risk / MRT / entropy terms of one pass' posterior; fills self.last_crf_*."""
        self.last_crf_risk = None
        self.last_crf_entropy = None
        self.last_crf_mrt = None
        self.last_token_ce = None
        if labels is not None:
            # args.token_ce_weight > 0 adds the token cross entropy of the emissions the CRF sees (TokenCrossEntropy, batch_mean:
            # the divisor of the CRF's mean NLL) to the loss and keeps it in self.last_token_ce; at the default 0 the step
            # launches nothing for it.
            if self.token_opt["weight"] > 0 and self.token_opt["head"] == "crf":
                token_ce = self.token_ce(emissions, labels, mask_u8, "batch_mean")
                self.last_token_ce = token_ce.detach()
                loss = loss + self.token_opt["weight"] * token_ce
            # args.crf_risk_weight > 0 adds the expected rate of wrong tags under the posterior (CRF.hamming_risk, token_mean) to
            # the loss and keeps it in self.last_crf_risk; at the default 0 the step launches nothing for it.
            risk_weight = _arg(self.args, "crf_risk_weight", 0.0)
            if risk_weight > 0:
                crf_risk = self.crf.hamming_risk(emissions, labels, mask=mask_u8, reduction="token_mean")
                self.last_crf_risk = crf_risk.detach()
                loss = loss + risk_weight * crf_risk
            # args.crf_mrt_weight > 0 adds minimum-risk training on the sentence-level entity F1 (CRF.minimum_risk, mean over
            # sentences): the hypothesis set is the decoded path above plus args.crf_mrt_samples (8) posterior samples
            # (CRF.sample: one dropout offset), the cost is 1 - F1 against the labels under args.entity_scheme
            # (metrics.sentence_f1_cost), the set's weights are softmax(args.crf_mrt_alpha * llh).  The mean risk stays in
            # self.last_crf_mrt; at the default 0 the step launches nothing for it and takes no offset.
            mrt_weight = _arg(self.args, "crf_mrt_weight", 0.0)
            if mrt_weight > 0:
                from ..metrics import sentence_f1_cost
                best = logits.device_tags
                if decoded is not None:  # the Viterbi tags come from the second stream
                    torch.cuda.current_stream().wait_event(decoded)
                    best.record_stream(torch.cuda.current_stream())
                drawn = self.crf.sample(emissions.detach(), mask_u8, n_samples=int(_arg(self.args, "crf_mrt_samples", 8)),
                                        return_logprob=False)
                hyp = torch.cat([best[:, None, :], drawn["tags"]], dim=1)
                cost = sentence_f1_cost(hyp, labels, mask_u8, self._entity_tables(emissions.device))
                crf_mrt = self.crf.minimum_risk(emissions, hyp, cost, mask=mask_u8, alpha=float(_arg(self.args, "crf_mrt_alpha", 1.0)),
                                                reduction="mean")
                self.last_crf_mrt = crf_mrt.detach()
                loss = loss + mrt_weight * crf_mrt
        # args.crf_entropy_weight != 0 adds weight * the posterior's sequence entropy per unmasked column (CRF.entropy, token_mean)
        # wherever a loss is formed -- positive minimises entropy, negative is a confidence penalty -- and keeps it in
        # self.last_crf_entropy; at the default 0 the step launches nothing for it.
        entropy_weight = _arg(self.args, "crf_entropy_weight", 0.0)
        if loss is not None and entropy_weight != 0:
            crf_entropy = self.crf.entropy(emissions, mask=mask_u8, reduction="token_mean")
            self.last_crf_entropy = crf_entropy.detach()
            loss = loss + entropy_weight * crf_entropy
        return loss

    # ------------------------------------------------------------------------------------------------
    def forward_consistent(self, input_ids=None, attention_mask=None, token_type_ids=None, labels=None, imagelabel=None,
                           images=None, aux_imgs=None, allowed_tags=None, token_to_word=None, prefix_mask=None, image_present=None, aux_present=None,
                           return_parts=False):
        """One training step's loss with a two-pass consistency term: the same batch goes through the encoder
        twice -- under two independent dropout masks (R-Drop), or once plain and once cut -- both passes are trained and a
        divergence between their predictive distributions joins the loss:

            1/2 (nll_1 + nll_2)   [args.consistency_ce = False: nll_1]
              + args.consistency_weight * divergence  +  alpha * img_tag_loss

        Arguments as ``forward`` (``prefix_mask`` / ``image_present`` / ``aux_present`` included: one slot mask, drawn once with
        args.modality_dropout, serves both passes); ``labels`` or ``allowed_tags`` is required (the nll is ``forward``'s, under args.crf_reduction).
        The visual prompt -- with args.vao its losses -- is computed once and serves both passes; ``alpha * img_tag_loss`` enters
        once.  Pass 1 is ``forward``'s pass.  Pass 2 runs the encoder again on the same prompt: in train mode under dropout masks
        of its own (as two ``forward`` calls draw them), and with args.consistency_aug ("span_cutoff" | "token_cutoff" |
        "dim_cutoff"; None = plain R-Drop) through `modules.augument.Cutoff` (args.aug_cutoff_ratio): the encoder sees the cut
        attention mask, while the head, the CRF and the divergence keep ``attention_mask`` -- a CRF needs its prefix mask and a
        cut column still has a label.
        args.consistency_level "token" (default): `engine.TokenDivergenceFunction` on the two emission tensors, args.consistency_kind
        ("sym_kl" | "js"), args.consistency_temperature (1.0), mean over the unmasked tokens.  "chain": `CRF.symmetric_kl` between
        the two posteriors over whole paths, 'token_mean'.  args.consistency_weight <= 0 (the default 0) skips the divergence; with
        args.consistency_ce = False as well pass 2 is not run.
        With args.word_pooling both passes pool onto the word axis and the divergence runs there; with args.layer_mix both read the
        mix; with args.fused_accumulation the two encoder nodes share the flat gradient buffers.  The Viterbi
        paths, ``entity_scorer.update``, ``last_*`` and the risk / MRT / entropy terms (args.crf_*_weight) come from pass 1 only.
        -> ``TokenClassifierOutput(loss, logits=pass-1 paths)``; with ``return_parts`` also a dict: ``nll`` (pass 1), ``nll_2``,
        ``divergence`` (unweighted, detached), ``emissions``, ``emissions_2`` -- None where a term was not computed."""
        if labels is None and allowed_tags is None:
            raise ValueError("forward_consistent forms a loss: it needs labels or allowed_tags")
        self._chain_only(allowed_tags is not None, "allowed_tags")
        opt = _consistency_options(self.args)
        self._chain_only(opt["level"] == "chain", "args.consistency_level='chain'")
        two = opt["weight"] > 0 or opt["ce"]
        # args.fused_accumulation: the two encoder nodes write / add into the flat gradient buffers, as in
        # TVNetSAModel.forward_with_cutoff; the sink goes back to its setting when that backward ends, or here if anything raises
        sink = self.bert.encoder.grad_sink if (_arg(self.args, "fused_accumulation") and torch.is_grad_enabled() and two) else None
        batch = (input_ids, attention_mask, token_type_ids, labels, imagelabel, images, aux_imgs, allowed_tags, token_to_word,
                 return_parts, prefix_mask, image_present, aux_present)
        if sink is None:
            return self._consistent_passes(opt, two, *batch)
        sink.begin_two_node_pass()
        try:
            return self._consistent_passes(opt, two, *batch)
        except BaseException:
            sink.end_two_node_pass()
            raise

    def _consistent_passes(self, opt, two, input_ids, attention_mask, token_type_ids, labels, imagelabel, images, aux_imgs, allowed_tags,
                           token_to_word, return_parts, prefix_mask=None, image_present=None, aux_present=None):
        word_mode = self._word_mode(token_to_word)
        prefix_guids, img_tag_loss, prompt_attention_mask = self._prompt_prologue(input_ids, attention_mask, imagelabel, images,
                                                                                  aux_imgs, prefix_mask, image_present, aux_present)
        self.bert.encoder.output_prefix_mass = bool(_arg(self.args, "output_prefix_mass"))
        bert_output = self.bert(input_ids=input_ids, attention_mask=prompt_attention_mask,
                                token_type_ids=token_type_ids, past_key_values=prefix_guids,
                                output_attentions=_arg(self.args, "output_attentions"), output_hidden_states=True,
                                return_dict=True, layer_mix=self.layer_mix, prefix_masked=self.last_prefix_slots is not None)
        self.last_prefix_mass = self.bert.encoder.last_prefix_mass if self.bert.encoder.output_prefix_mass else None
        index = None
        if word_mode is not None:
            index, attention_mask, labels, allowed_tags = self._word_targets(attention_mask, token_to_word, labels, allowed_tags)
        emissions = self._emissions(_head_state(bert_output, self.layer_mix), index, word_mode)
        mask_u8 = attention_mask.to(torch.uint8)
        logits, decoded = self._decode(emissions, mask_u8, labels)
        self.last_tag_marginals = self.crf.marginals(emissions.detach(), mask_u8) \
            if _arg(self.args, "output_tag_marginals") else None
        nll = self._crf_nll(emissions, mask_u8, labels, allowed_tags)
        parts = {"nll": nll, "nll_2": None, "divergence": None, "emissions": emissions, "emissions_2": None}
        loss = nll
        if two:
            self.bert.encoder.output_prefix_mass = False  # (pass 1 filled last_prefix_mass)
            if opt["aug"] is None:
                hidden_2 = _head_state(self.bert(input_ids=input_ids, attention_mask=prompt_attention_mask,
                                                 token_type_ids=token_type_ids, past_key_values=prefix_guids,
                                                 output_hidden_states=True, return_dict=True, layer_mix=self.layer_mix,
                                                 prefix_masked=self.last_prefix_slots is not None),
                                       self.layer_mix)
            else:
                from ..modules.augument import Cutoff
                cutoff = Cutoff(input_ids=input_ids, token_type_ids=token_type_ids, attention_masks=prompt_attention_mask,
                                prefix_guids=prefix_guids, args=self.args, model=self.bert, layer_mix=self.layer_mix)
                hidden_2 = cutoff._training_step_with_cutoff(opt["aug"])[0 if self.layer_mix is None else 2]
            emissions_2 = self._emissions(hidden_2, index, word_mode)
            parts["emissions_2"] = emissions_2
            if opt["ce"]:
                parts["nll_2"] = self._crf_nll(emissions_2, mask_u8, labels, allowed_tags)
                loss = 0.5 * (nll + parts["nll_2"])
            if opt["weight"] > 0:
                if opt["level"] == "token":  # the weight rides in the kernel
                    div = engine.TokenDivergenceFunction.apply(emissions, emissions_2, mask_u8, opt["kind"], opt["temperature"],
                                                               "token_mean", opt["weight"])
                else:
                    div = opt["weight"] * self.crf.symmetric_kl(emissions, emissions_2, mask_u8, reduction="token_mean")
                loss = loss + div
                if return_parts:
                    parts["divergence"] = div.detach() / opt["weight"]
        extra = _arg(self.args, "alpha", 0.0) * img_tag_loss
        if torch.is_tensor(extra) or extra != 0:
            loss = loss + extra
        loss = self._posterior_terms(loss, emissions, mask_u8, labels, logits, decoded)
        if decoded is not None:
            torch.cuda.current_stream().wait_event(decoded)  # (as in `forward`: the decode reads the CRF parameters)
        out = TokenClassifierOutput(loss=loss, logits=logits, attentions=bert_output.attentions)
        return (out, parts) if return_parts else out

    # ------------------------------------------------------------------------------------------------
    def _word_mode(self, token_to_word):
        """args.word_pooling when this call runs on the word axis (`mtvaf_amd.words`), else None: the head then reads pieces, as it
        always did.  The switch without a map at call time is an error, not a quiet piece-level run."""
        mode = _arg(self.args, "word_pooling", None)
        if mode is None:
            return None
        if token_to_word is None:
            raise ValueError(f"args.word_pooling={mode!r}: this model's head runs over words and needs token_to_word [B,S] "
                             "(mtvaf_amd.spans.batch_token_to_word, or spans.word_starts_from_labels) with every call")
        return mode

    def _word_axis(self, hidden, attention_mask, token_to_word, word_mask=None):
        """The prologue's last step of the ``predict*`` methods: (hidden, attention_mask) as they are, or -- args.word_pooling and
        a map -- the pooled hidden states [B,W,H] and the word axis' mask.  ``word_mask`` picks word columns on the piece axis:
        on the word axis every column is one, so it is refused together with ``token_to_word``."""
        mode = self._word_mode(token_to_word)
        if mode is None:
            return hidden, attention_mask
        if word_mask is not None:
            raise ValueError("word_mask marks the word columns of the piece axis: with token_to_word every column is a word; "
                             "pass one of the two")
        from ..words import build_word_index
        index = build_word_index(attention_mask, token_to_word, _arg(self.args, "max_words", None))
        self.last_word_index = index
        return engine.WordPoolFunction.apply(hidden, index, mode), index.word_mask

    def _calibration_labels(self, kind, labels, token_to_word):
        """The gold labels `self.calibration_scorer` chunks for a ``predict*`` call that scores ``kind``, on the axis the head ran
        on (args.word_pooling: `words.word_labels` over the call's word index); None when nothing is to be scored -- no labels,
        no scorer, or a scorer of the other kind."""
        if labels is None or self.calibration_scorer is None or _arg(self.args, "score_calibration") != kind:
            return None
        if self._word_mode(token_to_word) is not None:
            from ..words import word_labels
            return word_labels(labels, self.last_word_index)
        return labels

    def _entity_tables(self, device):
        """The tagging scheme of `predict` on ``device`` (args.entity_scheme, default "seqeval") over the trainer's label map
        (label_list enumerated from 1, MTVAF_training.py:369), plus the lookup of the structural predicted labels: built once."""
        scheme = _arg(self.args, "entity_scheme", "seqeval")
        key = (torch.device(device), scheme)
        if self._predict_tables is None or self._predict_tables[0] != key:
            from ..metrics import entity_device_tables, entity_tables, structural_labels
            label_map = {label: i for i, label in enumerate(self.label_list, 1)}
            t = entity_device_tables(entity_tables(label_map, scheme), device)
            structural = structural_labels(label_map)
            t["structural"] = torch.tensor([n in structural for n in t["names"]], dtype=torch.bool, device=device)
            self._predict_tables = (key, t)
        return self._predict_tables[1]

    def predict(self, input_ids, attention_mask, token_type_ids, images=None, aux_imgs=None, word_mask=None, token_to_word=None,
                prefix_mask=None, image_present=None, aux_present=None, labels=None):
        """Inference end to end with no host sync, in eval mode whatever mode the module is in: visual prompt -> encoder -> fc ->
        Viterbi -> `CRF.entities`.  Chunked columns: the run of attention_mask from column 1, minus the columns whose PREDICTED
        label is structural (`mtvaf_amd.metrics.structural_labels`: PAD, X, [CLS], [SEP]), and only those of ``word_mask``
        [B,S] when it is given (e.g. first sub-tokens).  args.entity_scheme ("seqeval" | "reference"), args.max_entities (32).
        -> the dict of `CRF.entities` (tags, lengths, entities, log_confidence, confidence, count) plus ``types``, the type
        names the entities' type indices refer to; `mtvaf_amd.metrics.entities_to_lists` turns it into Python lists.
        With args.word_pooling, ``token_to_word`` int32 [B,S] (as in `forward`) puts fc, the decoder and `CRF.entities` on the word
        axis: tags [B,W] and entity columns are WORD columns (``self.last_word_index``); ``word_mask`` is refused beside it.  The
        other ``predict_*`` methods take it the same way.  ``prefix_mask`` / ``image_present`` / ``aux_present``: as `forward` (eval
        mode: args.modality_dropout never drops here); every ``predict_*`` method takes them.
        ``labels`` [B,S] with args.score_calibration = "entities": the call then adds its entities and their log_confidence to
        ``self.calibration_scorer`` (`mtvaf_amd.metrics.CalibrationScorer.update_entities`; gold columns: 1 .. L-1 minus the gold X
        / [SEP]); the returned dict is the same either way, and without labels or the switch nothing more is launched.
        This and the other ``predict_*`` methods read the weights the module holds: to evaluate the averaged weights of a run with
        ``args.ema_decay``, call them inside ``with optimizer.averaged_parameters():`` (`mtvaf_amd.optim.AdamW`)."""
        # (an eval pass still reserves dropout offsets: the counter is put back, so a training run draws the same masks with or
        # without predictions in between)
        was_training, mass, offset = self.training, self.bert.encoder.output_prefix_mass, engine.RNG.offset
        self.eval()
        try:
            with torch.no_grad():
                if _arg(self.args, "use_prefix"):
                    prefix_guids, _, _ = self.get_visual_prompt(images, aux_imgs, None, vao=False)
                    prompt_attention_mask = _prompt_attention_mask(self, attention_mask, prefix_guids[0][0].shape[2], prefix_mask,
                                                                   image_present, aux_present)
                else:
                    _no_prefix(self, prefix_mask, image_present, aux_present)
                    prefix_guids, prompt_attention_mask = None, attention_mask
                self.bert.encoder.output_prefix_mass = False
                bert_output = self.bert(input_ids=input_ids, attention_mask=prompt_attention_mask, token_type_ids=token_type_ids,
                                        past_key_values=prefix_guids, output_attentions=False, output_hidden_states=True,
                                        return_dict=True, layer_mix=self.layer_mix, prefix_masked=self.last_prefix_slots is not None)
                hidden, attention_mask = self._word_axis(_head_state(bert_output, self.layer_mix), attention_mask, token_to_word,
                                                         word_mask)
                emissions = engine.LinearFunction.apply(hidden, self.fc.weight, self.fc.bias, False)
                mask_u8 = attention_mask.to(torch.uint8)
                # (the softmax head: per-token maxima; self.crf is then the chain of zero buffers, whose segment posteriors are
                # the sums of the token log-probabilities)
                tags, _ = self._token_tags(emissions, mask_u8) if self.token_opt["head"] == "softmax" \
                    else self.crf.decode_packed(emissions, mask_u8)
                t = self._entity_tables(emissions.device)
                keep = torch.zeros_like(mask_u8, dtype=torch.bool)
                keep[:, 1:] = torch.cumprod(mask_u8[:, 1:], dim=1).bool()  # from column 1 up to the first 0
                keep &= ~t["structural"][tags.clamp(0, t["C"] - 1).long()]
                if word_mask is not None:
                    keep &= word_mask.to(keep.device) != 0
                out = self.crf.entities(emissions, mask_u8, t, tags=tags, keep=keep,
                                        max_entities=_arg(self.args, "max_entities", 32))
                gold = self._calibration_labels("entities", labels, token_to_word)
                if gold is not None:
                    self.calibration_scorer.update_entities(out["entities"], out["log_confidence"], gold.to(emissions.device),
                                                            mask_u8)
        finally:
            self.bert.encoder.output_prefix_mass = mass
            engine.RNG.offset = offset
            self.train(was_training)
        out["types"] = t["types"]
        return out

    def predict_constrained(self, input_ids, attention_mask, token_type_ids, images=None, aux_imgs=None, word_mask=None,
                            allowed=None, token_to_word=None, prefix_mask=None, image_present=None, aux_present=None, labels=None):
        """`predict` with the decoder searching only among the tag sequences that the input's layout permits, instead of decoding
        freely and dropping the columns whose predicted label is structural afterwards: the same prologue (visual prompt ->
        encoder -> fc, eval mode, no host sync, dropout counter put back), then `CRF.decode_constrained` over ``allowed`` int64
        [B,S] (`mtvaf_amd.constraints`; None: `structural_sets` of the trainer's label map, the attention mask and ``word_mask``
        -- [CLS] / [SEP] at the ends, X on the columns outside ``word_mask``, no structural tag on a word column), then
        `CRF.entities` on those tags by `predict`'s column rule.  -> `predict`'s dict.  The reported confidence stays the
        posterior of the decoded segment under the UNCONSTRAINED chain, p(y_b..y_e | x), not conditioned on the sets.
        ``labels`` with args.score_calibration = "entities": as `predict`."""
        self._chain_only(True, "predict_constrained")
        # (the prologue is `predict`'s, restated: that method is left as it is)
        was_training, mass, offset = self.training, self.bert.encoder.output_prefix_mass, engine.RNG.offset
        self.eval()
        try:
            with torch.no_grad():
                if _arg(self.args, "use_prefix"):
                    prefix_guids, _, _ = self.get_visual_prompt(images, aux_imgs, None, vao=False)
                    prompt_attention_mask = _prompt_attention_mask(self, attention_mask, prefix_guids[0][0].shape[2], prefix_mask,
                                                                   image_present, aux_present)
                else:
                    _no_prefix(self, prefix_mask, image_present, aux_present)
                    prefix_guids, prompt_attention_mask = None, attention_mask
                self.bert.encoder.output_prefix_mass = False
                bert_output = self.bert(input_ids=input_ids, attention_mask=prompt_attention_mask, token_type_ids=token_type_ids,
                                        past_key_values=prefix_guids, output_attentions=False, output_hidden_states=True,
                                        return_dict=True, layer_mix=self.layer_mix, prefix_masked=self.last_prefix_slots is not None)
                hidden, attention_mask = self._word_axis(_head_state(bert_output, self.layer_mix), attention_mask, token_to_word,
                                                         word_mask)
                emissions = engine.LinearFunction.apply(hidden, self.fc.weight, self.fc.bias, False)
                mask_u8 = attention_mask.to(torch.uint8)
                if allowed is None:
                    from ..constraints import structural_sets
                    allowed = structural_sets({label: i for i, label in enumerate(self.label_list, 1)}, attention_mask, word_mask)
                tags, _ = self.crf.decode_constrained(emissions, allowed.to(emissions.device), mask_u8)
                t = self._entity_tables(emissions.device)
                keep = torch.zeros_like(mask_u8, dtype=torch.bool)
                keep[:, 1:] = torch.cumprod(mask_u8[:, 1:], dim=1).bool()  # from column 1 up to the first 0
                keep &= ~t["structural"][tags.clamp(0, t["C"] - 1).long()]
                if word_mask is not None:
                    keep &= word_mask.to(keep.device) != 0
                out = self.crf.entities(emissions, mask_u8, t, tags=tags, keep=keep,
                                        max_entities=_arg(self.args, "max_entities", 32))
                gold = self._calibration_labels("entities", labels, token_to_word)
                if gold is not None:
                    self.calibration_scorer.update_entities(out["entities"], out["log_confidence"], gold.to(emissions.device),
                                                            mask_u8)
        finally:
            self.bert.encoder.output_prefix_mass = mass
            engine.RNG.offset = offset
            self.train(was_training)
        out["types"] = t["types"]
        return out

    def predict_posteriors(self, input_ids, attention_mask, token_type_ids, images=None, aux_imgs=None, word_mask=None,
                           threshold=0.5, token_to_word=None, prefix_mask=None, image_present=None, aux_present=None, labels=None):
        """`predict_constrained` plus the posterior of every chunk EVENT (`CRF.chunk_posteriors`): the same prologue and the same
        layout sets (`structural_sets` of the trainer's label map, the attention mask and ``word_mask``), the posteriors
        conditional on them.  Kept columns: the word columns between [CLS] and [SEP] (columns 1 .. L-2, and only those of
        ``word_mask`` when it is given) -- the columns `predict_constrained` chunks.  args.max_entity_width (8): the widest span,
        in kept columns, 1..16.  No host sync.
        -> dict: ``decoded`` = `predict_constrained`'s dict, unchanged, plus ``chunk_log_conf`` [B,E], the log probability that
        the decoded entity is a chunk of the answer (0 in unused slots, -inf for an entity wider than max_entity_width);
        ``log_post`` [B,S,W,n_types] and ``logz_a`` [B] of `CRF.chunk_posteriors`; ``keep`` [B,S]; ``selected`` = the spans whose
        posterior is >= ``threshold`` in `predict`'s entities / log_confidence / confidence / count format, ordered by end column,
        then start (`CRF.chunks_above`; args.max_entities); ``types``.  Two overlapping chunks exclude each other, so with
        ``threshold > 0.5`` the selected spans of a sentence cannot overlap.  `mtvaf_amd.metrics.posteriors_to_lists` makes
        Python lists of it.
        ``labels`` [B,S] with args.score_calibration = "events": the call then adds every finite event of ``log_post`` to
        ``self.calibration_scorer`` (`mtvaf_amd.metrics.CalibrationScorer.update_events`, gold chunked over ``keep``); the returned
        dict is the same either way, and without labels or the switch nothing more is launched."""
        self._chain_only(True, "predict_posteriors")
        # (the prologue is `predict`'s, restated: that method is left as it is)
        was_training, mass, offset = self.training, self.bert.encoder.output_prefix_mass, engine.RNG.offset
        self.eval()
        try:
            with torch.no_grad():
                if _arg(self.args, "use_prefix"):
                    prefix_guids, _, _ = self.get_visual_prompt(images, aux_imgs, None, vao=False)
                    prompt_attention_mask = _prompt_attention_mask(self, attention_mask, prefix_guids[0][0].shape[2], prefix_mask,
                                                                   image_present, aux_present)
                else:
                    _no_prefix(self, prefix_mask, image_present, aux_present)
                    prefix_guids, prompt_attention_mask = None, attention_mask
                self.bert.encoder.output_prefix_mass = False
                bert_output = self.bert(input_ids=input_ids, attention_mask=prompt_attention_mask, token_type_ids=token_type_ids,
                                        past_key_values=prefix_guids, output_attentions=False, output_hidden_states=True,
                                        return_dict=True, layer_mix=self.layer_mix, prefix_masked=self.last_prefix_slots is not None)
                hidden, attention_mask = self._word_axis(_head_state(bert_output, self.layer_mix), attention_mask, token_to_word,
                                                         word_mask)
                emissions = engine.LinearFunction.apply(hidden, self.fc.weight, self.fc.bias, False)
                mask_u8 = attention_mask.to(torch.uint8)
                from ..constraints import structural_sets
                allowed = structural_sets({label: i for i, label in enumerate(self.label_list, 1)}, attention_mask,
                                          word_mask).to(emissions.device)
                tags, _ = self.crf.decode_constrained(emissions, allowed, mask_u8)
                t = self._entity_tables(emissions.device)
                run = torch.zeros_like(mask_u8, dtype=torch.bool)
                run[:, 1:] = torch.cumprod(mask_u8[:, 1:], dim=1).bool()  # from column 1 up to the first 0
                keep = run & ~t["structural"][tags.clamp(0, t["C"] - 1).long()]
                if word_mask is not None:
                    keep &= word_mask.to(keep.device) != 0
                decoded = self.crf.entities(emissions, mask_u8, t, tags=tags, keep=keep,
                                            max_entities=_arg(self.args, "max_entities", 32))
                # the word columns between [CLS] and [SEP], whatever was decoded there: the same columns, since the sets leave no
                # structural tag on a word column and nothing else on the others
                lens = torch.cumprod(mask_u8.long(), dim=1).sum(dim=1, keepdim=True)
                col = torch.arange(mask_u8.shape[1], device=mask_u8.device)[None, :]
                keep_w = (col >= 1) & (col < lens - 1)
                if word_mask is not None:
                    keep_w &= word_mask.to(keep_w.device) != 0
                log_post, logz_a = self.crf.chunk_posteriors(emissions, mask_u8, t, keep=keep_w, allowed=allowed,
                                                             max_width=_arg(self.args, "max_entity_width", 8))
                decoded["chunk_log_conf"] = self.crf.entity_chunk_confidence(decoded["entities"], log_post, keep_w)
                selected = self.crf.chunks_above(log_post, keep_w, threshold, _arg(self.args, "max_entities", 32))
                gold = self._calibration_labels("events", labels, token_to_word)
                if gold is not None:
                    self.calibration_scorer.update_events(log_post, keep_w, gold.to(emissions.device), mask_u8)
        finally:
            self.bert.encoder.output_prefix_mass = mass
            engine.RNG.offset = offset
            self.train(was_training)
        decoded["types"] = t["types"]
        return {"decoded": decoded, "log_post": log_post, "logz_a": logz_a, "keep": keep_w, "selected": selected,
                "types": t["types"]}

    def predict_nbest(self, input_ids, attention_mask, token_type_ids, images=None, aux_imgs=None, word_mask=None, nbest=None,
                      token_to_word=None, prefix_mask=None, image_present=None, aux_present=None):
        """`predict` with the ``nbest`` best tag sequences of every sentence instead of the best one (args.nbest, default 4; 1..8):
        the same prologue (visual prompt -> encoder -> fc, eval mode, no host sync, dropout counter put back), then
        `CRF.decode_nbest`, then every hypothesis through `CRF.entities` as one batch of B * K rows against the repeated emissions
        -- each hypothesis gets its entities and their posterior confidence in `predict`'s format and by `predict`'s column rule.
        -> dict: tags [B,K,S], scores / logprob [B,K], n_paths [B] (`CRF.decode_nbest`); lengths / count [B,K], entities
        [B,K,E,3], log_confidence / confidence [B,K,E] (`CRF.entities`), ``types``.  Hypothesis 0 is `predict`'s answer; ranks >=
        n_paths have no entities."""
        self._chain_only(True, "predict_nbest")
        K = int(_arg(self.args, "nbest", 4) if nbest is None else nbest)
        # (the prologue is `predict`'s, restated: that method is left as it is)
        was_training, mass, offset = self.training, self.bert.encoder.output_prefix_mass, engine.RNG.offset
        self.eval()
        try:
            with torch.no_grad():
                if _arg(self.args, "use_prefix"):
                    prefix_guids, _, _ = self.get_visual_prompt(images, aux_imgs, None, vao=False)
                    prompt_attention_mask = _prompt_attention_mask(self, attention_mask, prefix_guids[0][0].shape[2], prefix_mask,
                                                                   image_present, aux_present)
                else:
                    _no_prefix(self, prefix_mask, image_present, aux_present)
                    prefix_guids, prompt_attention_mask = None, attention_mask
                self.bert.encoder.output_prefix_mass = False
                bert_output = self.bert(input_ids=input_ids, attention_mask=prompt_attention_mask, token_type_ids=token_type_ids,
                                        past_key_values=prefix_guids, output_attentions=False, output_hidden_states=True,
                                        return_dict=True, layer_mix=self.layer_mix, prefix_masked=self.last_prefix_slots is not None)
                hidden, attention_mask = self._word_axis(_head_state(bert_output, self.layer_mix), attention_mask, token_to_word,
                                                         word_mask)
                emissions = engine.LinearFunction.apply(hidden, self.fc.weight, self.fc.bias, False)
                mask_u8 = attention_mask.to(torch.uint8)
                out = self.crf.decode_nbest(emissions, mask_u8, nbest=K)
                B, _, S = out["tags"].shape
                tags = out["tags"].view(B * K, S)
                t = self._entity_tables(emissions.device)
                keep = torch.zeros_like(mask_u8, dtype=torch.bool)
                keep[:, 1:] = torch.cumprod(mask_u8[:, 1:], dim=1).bool()  # from column 1 up to the first 0
                if word_mask is not None:
                    keep &= word_mask.to(keep.device) != 0
                keep = keep.repeat_interleave(K, dim=0) & ~t["structural"][tags.clamp(0, t["C"] - 1).long()]
                exists = torch.arange(K, device=keep.device)[None, :] < out["n_paths"][:, None]
                keep &= exists.reshape(B * K, 1)  # a rank without a path chunks nothing
                ent = self.crf.entities(emissions.repeat_interleave(K, dim=0), mask_u8.repeat_interleave(K, dim=0), t, tags=tags,
                                        keep=keep, max_entities=_arg(self.args, "max_entities", 32))
        finally:
            self.bert.encoder.output_prefix_mass = mass
            engine.RNG.offset = offset
            self.train(was_training)
        for k in ("lengths", "entities", "log_confidence", "confidence", "count"):
            out[k] = ent[k].view(B, K, *ent[k].shape[1:])
        out["types"] = t["types"]
        return out

    # ------------------------------------------------------------------------------------------------
    def _region_features(self, images, aux_imgs):
        """-> (feats [B,4,F], [aux feats [B,4,F]]).  Accepts raw images (through the frozen ResNet,
        bert_model.py:536-539) or pre-extracted pyramid features [B,F,2,2] / [B,4,F] (aux: [B,n,...])."""
        bsz = images.size(0)
        L = self.prefix_len if self.prefix_len == 4 else 4  # Linear(3840, .) fixes prefix_len = 4
        raw = images.dim() == 4 and images.shape[1] == 3
        if raw:
            if self.image_model is None:
                raise RuntimeError("raw images were passed but the model was built without args.resnet_root")
            pyr, aux_pyr = self.image_model(images, aux_imgs)
            feats = torch.cat(pyr, dim=1).view(bsz, L, -1)
            aux = [torch.cat(a, dim=1).view(bsz, L, -1) for a in (aux_pyr or [])]
            return feats.float(), [a.float() for a in aux]
        feats = images.reshape(bsz, L, -1).float()
        aux = []
        if aux_imgs is not None:
            aux = [aux_imgs[:, i].reshape(bsz, L, -1).float() for i in range(aux_imgs.shape[1])]
        return feats, aux

    def get_visual_prompt(self, images, aux_imgs, imagelabel, vao=True, present=None):
        """reference: models/bert_model.py:534-588.  Returns (list of num_layers (K, V) [B,NH,P,64],
        img_tag_loss, [aux_img_tag_loss]).  ``vao=False`` (`predict`: there are no image labels at inference) leaves the VAO
        losses of args.vao out.  ``present`` [images, B] fp32 (1 / 0; None: every sentence has every image): the image-tag loss of
        image k is the mean over the sentences that HAVE it -- one without contributes nothing and is not counted in the divisor
        (0 when no sentence has it); all ones gives the bits of None."""
        feats, aux = self._region_features(images, aux_imgs)
        bsz, L, Fd = feats.shape
        cfg = self.bert.config
        hidden = cfg.hidden_size
        NI = 1 + len(aux)
        x = torch.stack([feats] + aux).reshape(NI * bsz * L, Fd)  # image-major rows
        e0, e2 = self.encoder_conv[0], self.encoder_conv[2]
        t = engine.LinearFunction.apply(x, e0.weight, e0.bias, True)
        enc = engine.LinearFunction.apply(t, e2.weight, e2.bias, False).view(NI, bsz, L, 8 * hidden)

        img_tag_loss = 0
        aux_img_tag_loss = []
        if _arg(self.args, "vao") and vao:
            means = engine.MeanLFunction.apply(enc.view(NI * bsz, L, 8 * hidden)).view(NI, bsz, 8 * hidden)
            target = imagelabel.to(means.device)
            heads = [self.img_classifier] + list(self.aux_img_classifier)
            if NI - 1 > len(self.aux_img_classifier):
                raise ValueError("the VAO branch supports at most 3 aux images (bert_model.py:459)")
            for k in range(NI):
                m = engine.dropout(means[k], self.img_dropout.p, self.training)
                z = engine.LinearFunction.apply(m, heads[k].weight, heads[k].bias, False)
                l = engine.KLFunction.apply(z, target, None if present is None else present[k])
                if k == 0:
                    img_tag_loss = l
                else:
                    aux_img_tag_loss.append(l)

        if self._packed_proj is None or not self._packed_proj.valid(self.projectors):
            self._packed_proj = _PackedLinears(self.projectors)
        pp = self._packed_proj
        NL = len(self.projectors)
        proj_params = [p for m in self.projectors for p in (m.weight, m.bias)]
        pkv = engine.PromptFunction.apply(enc, pp.w, pp.b, NL, *proj_params)
        return PrefixKV(pkv, cfg.num_attention_heads, hidden // cfg.num_attention_heads), img_tag_loss, aux_img_tag_loss



# ====================================================================================================
def flatten(x):
    """reference: models/bert_model.py:113-124"""
    if x.dim() == 2:
        return x.reshape(x.shape[0] * x.shape[1])
    if x.dim() == 3:
        return x.reshape(x.shape[0] * x.shape[1], x.shape[2])
    raise Exception()


def reconstruct(x, ref):
    """reference: models/bert_model.py:127-138"""
    if x.dim() == 1:
        return x.view(ref.shape[0], ref.shape[1])
    if x.dim() == 2:
        return x.view(ref.shape[0], ref.shape[1], x.shape[1])
    raise Exception()


class TVNetSAModel(nn.Module):
    """Span-extraction variant (reference models/bert_model.py:192-414): the same prefix-fused encoder, a
    start/end extraction head (``binary_affine``) trained with distant cross entropy, and a span classifier
    (gather the span's tokens -> ``unary_affine`` self-attention pooling -> ``dense``+tanh -> ``classifier``).
    Same constructor, ``forward`` / ``extraction`` / ``classification`` / ``get_visual_prompt`` signatures and
    parameter names as the reference, so ``modules/train.py::SATrainer`` drives it unchanged.

    The reference reads the widest span (``JR``) and the valid-token count back to the host inside
    ``get_span_representation`` (:160-165); here they stay in a device-side index block
    (``mtvaf_span_index``), so a training step of this model has no host sync either.

    ``augument=True`` runs the cutoff augmentation of ``modules/augument.py`` (``mtvaf_amd.modules.augument``);
    ``forward_with_cutoff`` is the trainer's whole ``do_aug`` step (plain pass + cut pass + consistency term) in one call.
    Not built (out of scope): the GCN branches (``gcn_layer_number`` / ``num_layers`` > 0,
    whose modules are missing from the reference checkout) and the structural probe."""

    def __init__(self, label_list, tokenizer, args, type_num=None, use_weight=False):
        super().__init__()
        self.args = args
        self.type_num = type_num
        self.tokenizer = tokenizer
        self.prefix_dim = _arg(args, "prefix_dim", 768)
        self.prefix_len = _arg(args, "prefix_len", 4)
        enc_cls = RobertaModel if "roberta" in args.bert_name else BertModel
        bert_config = _arg(args, "bert_config", None)
        self.bert = enc_cls(bert_config) if bert_config is not None else enc_cls.from_pretrained(args.bert_name)
        self.bert.skip_pooler = True  # pooler_output only feeds the (unbuilt) GCN branch (:349)
        self.layer_mix = _layer_mix(args, self.bert)  # args.layer_mix: the heads read a learned mix of the hidden states
        hidden = self.bert.config.hidden_size
        self.dense = nn.Linear(hidden, hidden)
        self.activation = nn.Tanh()
        self.unary_affine = nn.Linear(hidden, 1)
        self.binary_affine = nn.Linear(hidden, 2)
        self.num_labels = len(label_list) + 1
        self.classifier = nn.Linear(hidden, 4)
        if _arg(args, "use_prefix"):
            small = _arg(args, "use_34") or _arg(args, "use_18")
            self.feat_dim = 960 if small else 3840
            if _arg(args, "resnet_root", None) is not None:
                self.image_model = ImageModel(use_152=_arg(args, "use_152"), use_101=_arg(args, "use_101"),
                                              use_34=_arg(args, "use_34"), use_18=_arg(args, "use_18"),
                                              resnet_root=args.resnet_root)
            else:
                self.image_model = None
            self.encoder_conv = nn.Sequential(nn.Linear(self.feat_dim, 800), nn.Tanh(), nn.Linear(800, 4 * 2 * hidden))
            self.projectors = nn.ModuleList([nn.Linear(4 * hidden * 2, 4)
                                             for _ in range(self.bert.config.num_hidden_layers)])
            self._packed_proj: Optional[_PackedLinears] = None
        self.fc = nn.Linear(hidden, self.num_labels)  # unused by forward, kept: it is in the reference's state_dict
        self.dropout = nn.Dropout(0.1)
        # args.score_spans: `predict` with gold terms adds its aspect counts to model.span_scorer on the device
        self.span_scorer = _span_scorer(args)
        if _arg(args, "gcn_layer_number", 0) > 0 or _arg(args, "num_layers", 0) > 0:
            raise NotImplementedError("the GCN branches are outside the accelerated path (their modules are not in "
                                      "the reference checkout either: models/bert_model.py:233-237)")
        if _arg(args, "use_probe"):
            raise NotImplementedError("the structural probe (probes/) is off the hot path and its import chain is "
                                      "broken in the reference (models/bert_model.py:238-245)")

    # ------------------------------------------------------------------------------------------------
    def forward(self, input_ids=None, attention_mask=None, token_type_ids=None, start_positions=None,
                end_positions=None, span_starts=None, span_ends=None, polarity_labels=None, label_masks=None,
                images=None, aux_imgs=None, valid_ids=None, adjacency_matrix=None, output_attention=False,
                augument=False, labels=None, adj_matrix=None, src_mask=None, aspect_mask=None, polaritys=None, prefix_mask=None, image_present=None, aux_present=None):
        """reference: models/bert_model.py:246-321 (use_probe / GCN branches excluded).  ``prefix_mask`` / ``image_present`` /
        ``aux_present``: as `TVNetSAModel2.forward`."""
        prefix_guids, prompt_attention_mask = self._prompt_prologue(input_ids, attention_mask, images, aux_imgs, True, prefix_mask, image_present, aux_present)
        loss, logits = self._loss_pass(prefix_guids, prompt_attention_mask, input_ids, attention_mask, token_type_ids,
                                       start_positions, end_positions, span_starts, span_ends, polarity_labels,
                                       label_masks, augument)
        return TokenClassifierOutput(loss=loss, logits=logits)

    def forward_with_cutoff(self, input_ids=None, attention_mask=None, token_type_ids=None, start_positions=None,
                            end_positions=None, span_starts=None, span_ends=None, polarity_labels=None, label_masks=None,
                            images=None, aux_imgs=None, valid_ids=None, adjacency_matrix=None, output_attention=False,
                            labels=None, adj_matrix=None, src_mask=None, aspect_mask=None, polaritys=None,
                            prefix_mask=None, image_present=None, aux_present=None, return_parts=False):
        """One training step's loss with the cutoff augmentation on -- what ``SATrainer._step`` does when ``mode ==
        "train" and args.do_aug`` (modules/train.py:412-455 with cal_cut_loss / js_div, :523-538): a plain pass, a cut
        pass (``args.aug_type`` / ``args.aug_cutoff_ratio``) and

            loss + aug_ce_loss * cutoff_loss + aug_js_loss * js_div(softmax(logits, 1), softmax(cutoff_logits, 1))

        ``args.aug_ce_loss`` / ``args.aug_js_loss`` default to 1.0 (MTVAF_training.py:245-246); a weight <= 0 drops its
        term and with both <= 0 the cut pass is not run.  ``args.aug_js_masked`` (new, default False): ``label_masks``
        keeps the padding slots out of the consistency term; False is the reference, where they take part.
        The visual prompt is computed once and serves both passes (``get_visual_prompt`` has no randomness, so this
        equals the reference's two computations; autograd sums the two prefix gradients in front of one backward of the
        generator).  In train mode the two passes draw independent dropout masks, as two ``forward`` calls do.
        -> ``TokenClassifierOutput(loss=combined, logits=plain logits)``; with ``return_parts`` also a dict: ``loss``
        (plain), ``cutoff_loss``, ``js`` (unweighted, detached), ``cutoff_logits`` -- None where a term was not computed."""
        w_ce, w_js = _arg(self.args, "aug_ce_loss", 1.0), _arg(self.args, "aug_js_loss", 1.0)
        # args.fused_accumulation (opt-in): the two encoder nodes of this step share the flat gradient buffers -- the first
        # one the backward runs writes them, the second adds into them -- instead of sending both to the allocate-and-accumulate
        # fallback.  The sink goes back to its setting when that backward ends, or here if anything below raises.
        sink = self.bert.encoder.grad_sink if (_arg(self.args, "fused_accumulation") and torch.is_grad_enabled()
                                               and (w_ce > 0 or w_js > 0)) else None
        if sink is None:
            return self._cutoff_passes(w_ce, w_js, input_ids, attention_mask, token_type_ids, start_positions, end_positions, span_starts,
                                       span_ends, polarity_labels, label_masks, images, aux_imgs, return_parts, prefix_mask, image_present, aux_present)
        sink.begin_two_node_pass()
        try:
            return self._cutoff_passes(w_ce, w_js, input_ids, attention_mask, token_type_ids, start_positions, end_positions, span_starts,
                                       span_ends, polarity_labels, label_masks, images, aux_imgs, return_parts, prefix_mask, image_present, aux_present)
        except BaseException:
            sink.end_two_node_pass()
            raise

    def _cutoff_passes(self, w_ce, w_js, input_ids, attention_mask, token_type_ids, start_positions, end_positions, span_starts,
                       span_ends, polarity_labels, label_masks, images, aux_imgs, return_parts, prefix_mask=None, image_present=None,
                       aux_present=None):
        prefix_guids, prompt_attention_mask = self._prompt_prologue(input_ids, attention_mask, images, aux_imgs, True, prefix_mask, image_present, aux_present)
        batch = (prompt_attention_mask, input_ids, attention_mask, token_type_ids, start_positions, end_positions,
                 span_starts, span_ends, polarity_labels, label_masks)
        loss, logits = self._loss_pass(prefix_guids, *batch, False)
        parts = {"loss": loss, "cutoff_loss": None, "js": None, "cutoff_logits": None}
        combined = loss
        if w_ce > 0 or w_js > 0:
            cutoff_loss, cutoff_logits = self._loss_pass(prefix_guids, *batch, True)
            parts.update(cutoff_loss=cutoff_loss, cutoff_logits=cutoff_logits)
            if w_ce > 0:
                combined = combined + w_ce * cutoff_loss
            if w_js > 0:
                mask = label_masks if _arg(self.args, "aug_js_masked") else None
                js = engine.JSConsistencyFunction.apply(logits, cutoff_logits, mask, float(w_js))  # the weight rides in the kernel
                combined = combined + js
                if return_parts:
                    parts["js"] = js.detach() / float(w_js)
        out = TokenClassifierOutput(loss=combined, logits=logits)
        return (out, parts) if return_parts else out

    def _prompt_prologue(self, input_ids, attention_mask, images, aux_imgs, second_stream, prefix_mask=None, image_present=None,
                         aux_present=None):
        """-> (prefix_guids, prompt_attention_mask): the visual prompt and the attention mask extended over its slots
        (:262-271; `_prompt_attention_mask`: the per-sentence slot mask enters here); (None, attention_mask) without ``use_prefix``."""
        if not _arg(self.args, "use_prefix"):
            _no_prefix(self, prefix_mask, image_present, aux_present)
            return None, attention_mask
        if second_stream:
            prefix_guids = _on_second_stream(lambda: self.get_visual_prompt(images, aux_imgs), (images, aux_imgs))
        else:
            prefix_guids = self.get_visual_prompt(images, aux_imgs)
        return prefix_guids, _prompt_attention_mask(self, attention_mask, prefix_guids[0][0].shape[2], prefix_mask, image_present,
                                                    aux_present)

    def _loss_pass(self, prefix_guids, prompt_attention_mask, input_ids, attention_mask, token_type_ids, start_positions,
                   end_positions, span_starts, span_ends, polarity_labels, label_masks, augument):
        """Encoder + both heads + the loss of :298-303 for one (plain or cut) pass -> (loss, logits [B,M,4])."""
        ae_logits, sequence_output = self._extract(prompt_attention_mask, input_ids, prefix_guids, token_type_ids,
                                                   augument)
        logits, ac_logits = self.classification(attention_mask=attention_mask, span_starts=span_starts,
                                                span_ends=span_ends, sequence_input=sequence_output)
        flat_polarity_labels = flatten(polarity_labels)
        flat_label_masks = flatten(label_masks).to(dtype=ac_logits.dtype)
        # :298-300  (start_loss + end_loss) / 2, both distant cross entropies in one node
        ae_loss = engine.DistantCEPairFunction.apply(ae_logits, start_positions, end_positions)
        ac_loss = engine.CrossEntropyFunction.apply(ac_logits, flat_polarity_labels)
        ac_loss = torch.sum(flat_label_masks * ac_loss) / flat_label_masks.sum()  # :303, the reference's scalar quirk
        return ae_loss + ac_loss, logits

    def _extract(self, prompt_attention_mask, input_ids, prefix_guids, token_type_ids, augument=False):
        if augument:
            # :333-343 -- the cut input replaces the plain pass (the reference still runs the plain encoder first
            # and throws its output away; only hidden_states[7] of it feeds the unbuilt probe)
            from ..modules.augument import Cutoff
            cutoff = Cutoff(input_ids=input_ids, token_type_ids=token_type_ids, attention_masks=prompt_attention_mask,
                            prefix_guids=prefix_guids, args=self.args, model=self.bert, layer_mix=self.layer_mix)
            last_hidden = cutoff._training_step_with_cutoff(self.args.aug_type)[0 if self.layer_mix is None else 2]
        else:
            last_hidden = _head_state(self.bert(input_ids=input_ids, attention_mask=prompt_attention_mask,
                                                token_type_ids=token_type_ids, past_key_values=prefix_guids,
                                                output_attentions=_arg(self.args, "output_attentions"), output_hidden_states=True,
                                                return_dict=True, layer_mix=self.layer_mix), self.layer_mix)
        sequence_output = engine.dropout(last_hidden, self.dropout.p, self.training)
        ae_logits = engine.LinearFunction.apply(sequence_output, self.binary_affine.weight, self.binary_affine.bias, False)
        return ae_logits, sequence_output

    def extraction(self, prompt_attention_mask, input_ids, prefix_guids, token_type_ids, augument=False, labels=None,
                   adj_matrix=None, src_mask=None, aspect_mask=None):
        """reference: models/bert_model.py:323-361 -> (start_logits [B,S], end_logits [B,S], sequence_output)."""
        ae_logits, sequence_output = self._extract(prompt_attention_mask, input_ids, prefix_guids, token_type_ids, augument)
        return ae_logits[..., 0], ae_logits[..., 1], sequence_output

    def classification(self, span_starts, span_ends, sequence_input, attention_mask):
        """reference: models/bert_model.py:363-376 -> (logits [B,M,4], ac_logits [B*M,4])."""
        M = span_starts.shape[1]
        index = engine.hip.span_index(attention_mask.to(torch.uint8).contiguous(), span_starts.contiguous().long(),
                                      span_ends.contiguous().long())
        pooled = engine.SpanPoolFunction.apply(sequence_input, self.unary_affine.weight, self.unary_affine.bias, index, M)
        pooled = engine.LinearFunction.apply(pooled, self.dense.weight, self.dense.bias, True)
        pooled = engine.dropout(pooled, self.dropout.p, self.training)
        ac_logits = engine.LinearFunction.apply(pooled, self.classifier.weight, self.classifier.bias, False)
        return reconstruct(ac_logits, span_starts), ac_logits

    # ------------------------------------------------------------------------------------------------
    def propose_spans(self, start_logits, end_logits=None, attention_mask=None, token_to_word=None, word_key=None):
        """Candidate spans for eval / predict, on the device and without a host sync: what the reference's trainer does on the
        host between ``extraction`` and ``classification`` (modules/train.py:382-410 around the eval branch of
        models/utils.py::span_annotate_candidates).  ``start_logits`` / ``end_logits`` [B,S] as ``extraction`` returns them
        (two columns of one tensor: read in place), or the ``[B,S,2]`` extraction logits alone with ``end_logits=None``.
        ``token_to_word`` [B,S]: token -> original word, -1 outside the word map (`mtvaf_amd.spans`); None: every token with
        ``attention_mask`` 1 is its own word.  ``word_key`` [B,S]: ids of the words' strings; None: de-duplication by position.
        Read from ``args`` with the reference's defaults: n_best_size 20, max_answer_length 12, logit_threshold 8.0,
        use_heuristics True, use_nms False, filter_type 'f1'.
        -> span_starts, span_ends, label_masks [B,n_best_size] int64, span_scores [B,n_best_size] fp32, count [B] int32."""
        if end_logits is None:
            ae = start_logits
        elif (start_logits.dim() == 2 and start_logits.shape == end_logits.shape and start_logits.stride() == end_logits.stride()
              and start_logits.stride(1) >= 2 and start_logits.stride(0) == start_logits.shape[1] * start_logits.stride(1)
              and start_logits.untyped_storage().data_ptr() == end_logits.untyped_storage().data_ptr()
              and end_logits.storage_offset() == start_logits.storage_offset() + 1):
            ae = start_logits.as_strided((*start_logits.shape, 2), (*start_logits.stride(), 1))
        else:
            ae = torch.stack((start_logits, end_logits), dim=-1)
        ae = ae.detach().float()
        if token_to_word is None:
            if attention_mask is None:
                raise ValueError("propose_spans: give attention_mask or token_to_word")
            token_to_word = _mask_word_map(attention_mask, ae.device)
        filter_type = _arg(self.args, "filter_type", "f1")
        if filter_type not in ("f1", "em"):
            raise ValueError(f"args.filter_type={filter_type!r}: expected 'f1' or 'em'")
        # 'em' drops later candidates of equal text: the de-duplication has done that already
        nms = 1 if _arg(self.args, "use_nms", False) and filter_type == "f1" else 0
        return engine.hip.span_propose(
            ae, token_to_word.to(device=ae.device, dtype=torch.int32).contiguous(),
            None if word_key is None else word_key.to(device=ae.device, dtype=torch.int32).contiguous(),
            n_best=_arg(self.args, "n_best_size", 20), max_len=_arg(self.args, "max_answer_length", 12),
            threshold=_arg(self.args, "logit_threshold", 8.0), use_heuristics=_arg(self.args, "use_heuristics", True), nms=nms)

    def predict(self, input_ids, attention_mask, token_type_ids, images=None, aux_imgs=None, token_to_word=None,
                word_key=None, gold=None, prefix_mask=None, image_present=None, aux_present=None):
        """Inference end to end with no host sync: visual prompt -> extraction logits -> `propose_spans` -> span classifier.
        -> dict: span_starts, span_ends, label_masks [B,n] int64, span_scores [B,n] fp32, logits [B,n,4] (polarity logits of
        every slot; padding slots have label_masks 0), start_logits / end_logits [B,S] the proposal read.
        ``gold``: dict ``starts, ends, classes, masks`` [B,G], the feature's start_indexes, end_indexes, polarity_labels and
        label_masks.  With ``args.score_spans`` the call then adds the batch's aspect counts to ``self.span_scorer`` (one more
        launch on the same stream, on the word map the proposal read) and the dict also holds pred_class, matched_gold [B,n]
        int32 (`SpanScorer.update`).  Without ``gold`` or without the switch nothing more is launched.
        The weights read are the ones the module holds: to evaluate the averaged weights of a run with ``args.ema_decay``, call
        this inside ``with optimizer.averaged_parameters():`` (`mtvaf_amd.optim.AdamW`)."""
        with torch.no_grad():
            prefix_guids, prompt_attention_mask = self._prompt_prologue(input_ids, attention_mask, images, aux_imgs, False, prefix_mask,
                                                                        image_present, aux_present)
            ae_logits, sequence_output = self._extract(prompt_attention_mask, input_ids, prefix_guids, token_type_ids)
            if gold is not None and self.span_scorer is not None and token_to_word is None:
                token_to_word = _mask_word_map(attention_mask, ae_logits.device)  # one map for proposal and score
            span_starts, span_ends, label_masks, span_scores, _ = self.propose_spans(
                ae_logits, None, attention_mask, token_to_word=token_to_word, word_key=word_key)
            logits, _ = self.classification(span_starts, span_ends, sequence_output, attention_mask)
        out = {"span_starts": span_starts, "span_ends": span_ends, "label_masks": label_masks, "span_scores": span_scores,
               "logits": logits, "start_logits": ae_logits[..., 0], "end_logits": ae_logits[..., 1]}
        if gold is not None and self.span_scorer is not None:
            out["pred_class"], out["matched_gold"] = self.span_scorer.update(
                out, gold["starts"], gold["ends"], gold["classes"], gold["masks"], token_to_word, word_key, return_slots=True)
        return out

    _region_features = TVNetSAModel2._region_features

    def get_visual_prompt(self, images, aux_imgs):
        """reference: models/bert_model.py:379-414 -> list of num_layers (K, V) [B,NH,P,64]."""
        feats, aux = self._region_features(images, aux_imgs)
        bsz, L, Fd = feats.shape
        cfg = self.bert.config
        hidden = cfg.hidden_size
        NI = 1 + len(aux)
        x = torch.stack([feats] + aux).reshape(NI * bsz * L, Fd)
        e0, e2 = self.encoder_conv[0], self.encoder_conv[2]
        t = engine.LinearFunction.apply(x, e0.weight, e0.bias, True)
        enc = engine.LinearFunction.apply(t, e2.weight, e2.bias, False).view(NI, bsz, L, 8 * hidden)
        if self._packed_proj is None or not self._packed_proj.valid(self.projectors):
            self._packed_proj = _PackedLinears(self.projectors)
        pp = self._packed_proj
        proj_params = [p for m in self.projectors for p in (m.weight, m.bias)]
        pkv = engine.PromptFunction.apply(enc, pp.w, pp.b, len(self.projectors), *proj_params)
        return PrefixKV(pkv, cfg.num_attention_heads, hidden // cfg.num_attention_heads)
