"""Host-side helpers for the unchanged reference trainer.

``modules/train.py:627-647`` (train), ``:722-735`` / ``:805-818`` (evaluate / test) rebuild ``y_true`` / ``y_pred`` for
seqeval with a B x S Python double loop over ``labels.to('cpu')``, ``attention_mask.to('cpu')`` and the decoded tag lists:
~4k interpreted iterations per step at bs 32 / S 128, more than the GPU needs for the whole forward pass in bf16 mode.
``label_sequences`` produces the same two lists of label-name lists with array operations: one packed device->host copy
(the ``DeferredTags`` of ``TVNetSAModel2.forward`` already holds the tags in pinned memory), boolean masks, one lookup.

Rule restated from the reference loop: per sentence, walk the columns from 1 (column 0 is ``[CLS]``) while
``attention_mask`` is 1 and stop at the first 0; keep a position unless its gold label is ``"X"`` or ``"[SEP]"``; emit
``label_map^-1[label]`` and ``label_map^-1[predicted tag]`` (id 0 reads ``"PAD"``)."""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from .modules.crf import DeferredTags


def _tags_array(logits, B: int, S: int) -> np.ndarray:
    """Decoded tags as a [B, S] int array (padded with 0 beyond each sentence's length)."""
    if isinstance(logits, DeferredTags):
        packed = logits.packed()
        if packed is not None:
            return np.where(packed[:, :S] < 0, 0, packed[:, :S])
    out = np.zeros((B, S), dtype=np.int64)
    for r, row in enumerate(logits):
        n = min(len(row), S)
        out[r, :n] = row[:n]
    return out


def label_sequences(labels: torch.Tensor, attention_mask: torch.Tensor, logits: Sequence[Sequence[int]],
                    label_map: Dict[str, int]) -> Tuple[List[List[str]], List[List[str]]]:
    """-> (y_true, y_pred) exactly as the loops of modules/train.py:627-647 / :722-735 / :805-818 build them."""
    lab = labels.detach().to("cpu").numpy()
    msk = attention_mask.detach().to("cpu").numpy().astype(bool)
    B, S = lab.shape
    tags = _tags_array(logits, B, S)
    id2 = {idx: name for name, idx in label_map.items()}
    id2[0] = "PAD"
    top = int(max(max(id2), int(lab.max(initial=0)), int(tags.max(initial=0))))
    names = np.array([id2.get(i, "PAD") for i in range(top + 1)], dtype=object)
    run = np.logical_and.accumulate(msk[:, 1:], axis=1)  # the reference breaks at the first mask 0
    skip = [label_map[n] for n in ("X", "[SEP]") if n in label_map]
    keep = run & ~np.isin(lab[:, 1:], skip)
    y_true = [names[lab[r, 1:][keep[r]]].tolist() for r in range(B)]
    y_pred = [names[tags[r, 1:][keep[r]]].tolist() for r in range(B)]
    return y_true, y_pred


# -------------------------------------------------------------------------------------------------
# Entity-level score on the device (csrc/entity.hip): the lists above never leave the GPU
# -------------------------------------------------------------------------------------------------
SCHEMES = ("seqeval", "reference")
_CHUNK_CLASSES = ("B", "I", "E", "S")


def entity_tables(label_map: Dict[str, int], scheme: str = "seqeval", skip: Sequence[str] = ("X", "[SEP]")) -> dict:
    """The tagging scheme as the tables `mtvaf_entity_counts` reads, filled from label NAMES.

    Ids run 0 .. C-1 with C = max id + 1; the id -> name list is `label_sequences`': id 0 and holes read ``"PAD"``.  Index C is the
    sentence boundary and behaves as ``'O'``.  ``start[p][c]`` / ``end[p][c]``: a chunk starts at a label c that follows p / ends
    at a label p that c follows.

    ``"reference"``: modules/eval_metrics.py::get_chunks / get_chunk_type.  O is the id ``label_map['O']`` alone; every other
    name has class ``name.split('-')[0]`` and type ``name.split('-')[-1]``; start = c is not O and (p is O or the types differ or
    class(c) == 'B'); end = p is not O and (c is O or the types differ or class(c) == 'B').

    ``"seqeval"``: seqeval's default-mode get_entities on prefix tags, restated (the package is not a dependency): tag =
    ``name[0]``, type = ``name[1:].split('-', 1)[-1] or '_'``; the predicates are the ones spelled out in DESIGN.md section 7.

    -> dict(C, names, types, primary, start, end, type_of, gold_skip): ``types`` the type names in counter order, ``primary[t]``
    whether a label of class B / I / E / S carries type t (the others are reported only when they have counts)."""
    if scheme not in SCHEMES:
        raise ValueError(f"scheme={scheme!r}: expected one of {SCHEMES}")
    if "O" not in label_map:
        raise ValueError("the label map has no 'O'")
    if min(label_map.values()) < 0:
        raise ValueError("negative label id")
    id2 = {idx: name for name, idx in label_map.items()}
    id2[0] = "PAD"
    C = max(id2) + 1
    names = [id2.get(i, "PAD") for i in range(C)]
    if scheme == "reference":
        o_id = label_map["O"]
        outside = [i == o_id for i in range(C)] + [True]
        klass = [n.split("-")[0] for n in names] + ["O"]
        kind = ["O" if outside[i] else names[i].split("-")[-1] for i in range(C)] + ["O"]

        def start(p, c):
            return not outside[c] and (outside[p] or kind[p] != kind[c] or klass[c] == "B")

        def end(p, c):
            return not outside[p] and (outside[c] or kind[p] != kind[c] or klass[c] == "B")
    else:
        klass = [n[0] for n in names] + ["O"]
        kind = [n[1:].split("-", 1)[-1] or "_" for n in names] + ["_"]
        end_pairs = {("B", "B"), ("B", "S"), ("B", "O"), ("I", "B"), ("I", "S"), ("I", "O")}
        start_pairs = {("E", "E"), ("E", "I"), ("S", "E"), ("S", "I"), ("O", "E"), ("O", "I")}

        def start(p, c):
            return (klass[c] in ("B", "S") or (klass[p], klass[c]) in start_pairs
                    or (klass[c] not in ("O", ".") and kind[p] != kind[c]))

        def end(p, c):
            return (klass[p] in ("E", "S") or (klass[p], klass[c]) in end_pairs
                    or (klass[p] not in ("O", ".") and kind[p] != kind[c]))
    types: List[str] = []
    for k in kind:
        if k not in types:
            types.append(k)
    carried = {kind[i] for i in range(C) if klass[i] in _CHUNK_CLASSES and not (scheme == "reference" and outside[i])}
    n = C + 1
    return dict(C=C, names=names, types=types, primary=[t in carried for t in types],
                start=np.array([[start(p, c) for c in range(n)] for p in range(n)], dtype=np.uint8),
                end=np.array([[end(p, c) for c in range(n)] for p in range(n)], dtype=np.uint8),
                type_of=np.array([types.index(k) for k in kind], dtype=np.int32),
                gold_skip=np.array([names[i] in skip for i in range(C)], dtype=np.uint8))


def structural_labels(label_map: Dict[str, int]) -> tuple:
    """The label names that are neither ``"O"`` nor of the form ``<class>-<type>``, plus ``"PAD"`` (first), in id order: for the
    reference's list ``("PAD", "X", "[CLS]", "[SEP]")``.  `TVNetSAModel2.predict` leaves the columns whose PREDICTED label is one
    of these out of the chunking (at inference there is no gold label to skip by)."""
    def chunked(name):
        klass, sep, kind = name.partition("-")
        return bool(klass and sep and kind)
    rest = [n for n, _ in sorted(label_map.items(), key=lambda kv: kv[1]) if n not in ("O", "PAD") and not chunked(n)]
    return ("PAD", *rest)


def entity_device_tables(tables: dict, device) -> dict:
    """The tables of `entity_tables` as `mtvaf_crf_entities` reads them, on ``device``: start / end [(C+1)^2] uint8, type_of
    [C+1] int32, plus n_types, types, names and C.  A dict that already holds tensors is returned as it is."""
    if torch.is_tensor(tables["start"]):
        return tables
    out = {k: torch.from_numpy(np.ascontiguousarray(tables[k])).reshape(-1).to(device) for k in ("start", "end", "type_of")}
    out.update(n_types=len(tables["types"]), types=list(tables["types"]), names=list(tables["names"]), C=tables["C"])
    if "gold_skip" in tables:  # what the counting kernels read besides (`sentence_f1_cost`)
        out["gold_skip"] = torch.from_numpy(np.ascontiguousarray(tables["gold_skip"])).reshape(-1).to(device)
    return out


def sentence_f1_cost(hyp_tags: torch.Tensor, gold: torch.Tensor, mask: torch.Tensor, tables: dict, return_counts: bool = False):
    """The entity-level cost of every hypothesis against its sentence's labels, on the device with no host sync (one
    `mtvaf_entity_counts_rows` launch): ``cost[b,k] = 1 - F1 = 1 - 2 c / (p + g)`` with p / g / c the predicted / gold / correct
    chunks of hypothesis k under `EntityScorer`'s counting rule, and 0 where ``p + g == 0`` (nothing to find, nothing found).

    ``hyp_tags`` int [B,K,S] (``CRF.sample`` / ``CRF.decode_nbest`` tags, -1 behind the sentence), ``gold`` [B,S] labels,
    ``mask`` [B,S]; ``tables``: the dict of `entity_tables` or of `entity_device_tables` (which carries ``gold_skip``), the way
    `EntityScorer` / `TVNetSAModel2._entity_tables` build them.  -> cost float32 [B,K]; with ``return_counts`` also the counts
    int32 [B,K,3].  The cost of MRT (`CRF.minimum_risk`); it carries no gradient."""
    from . import hip
    if hyp_tags.dim() != 3 or gold.dim() != 2 or hyp_tags.shape[0] != gold.shape[0] or hyp_tags.shape[2] != gold.shape[1]:
        raise ValueError(f"sentence_f1_cost: hypotheses {tuple(hyp_tags.shape)} do not fit gold {tuple(gold.shape)}: expected "
                         "[B, K, S] and [B, S]")
    B, K, S = hyp_tags.shape
    t = entity_device_tables(tables, hyp_tags.device)
    if "gold_skip" not in t:
        raise ValueError("sentence_f1_cost: the tables carry no gold_skip (build them with entity_tables / entity_device_tables)")
    hyp = hyp_tags if hyp_tags.dtype == torch.int32 else hyp_tags.to(torch.int32)
    mask_u8 = mask if mask.dtype == torch.uint8 else mask.to(torch.uint8)
    gold = gold if gold.dtype == torch.int64 else gold.to(torch.int64)
    rows = hip.entity_counts_rows(hyp.contiguous().view(B * K, S), gold.contiguous(), mask_u8.contiguous(), t["start"], t["end"],
                                  t["type_of"], t["gold_skip"], t["n_types"], group=K).view(B, K, 3)
    p, g, c = (rows[..., i].to(torch.float32) for i in range(3))
    cost = torch.where(p + g > 0, 1.0 - 2.0 * c / (p + g).clamp(min=1.0), torch.zeros_like(p))
    return (cost, rows) if return_counts else cost


def entities_to_lists(result: dict, types: Sequence[str]) -> List[List[dict]]:
    """The dict of `CRF.entities` / `TVNetSAModel2.predict` -> per sentence a list of ``{"start", "end", "type", "confidence"}``
    (token columns, inclusive end; ``types`` names the type indices), ordered by end column: at most ``max_entities`` per sentence.
    ONE device->host copy -- the only part of the inference path that waits for the GPU."""
    ents, conf, count = result["entities"], result["confidence"], result["count"]
    B, E = conf.shape
    packed = torch.cat([ents.reshape(B, E * 3).double(), conf.double(), count.reshape(B, 1).double()], dim=1).cpu().numpy()
    out = []
    for row in packed:
        n = min(int(row[-1]), E)
        e, c = row[:E * 3].reshape(E, 3).astype(np.int64), row[E * 3:E * 4]
        out.append([{"start": int(e[k, 0]), "end": int(e[k, 1]), "type": types[int(e[k, 2])], "confidence": float(c[k])}
                    for k in range(n)])
    return out


def posteriors_to_lists(result: dict) -> List[dict]:
    """The dict of `TVNetSAModel2.predict_posteriors` -> per sentence ``{"decoded": [...], "selected": [...]}``: the decoded
    entities as `entities_to_lists` gives them plus ``"chunk_confidence"`` (the posterior of the chunk event, 0.0 for an entity
    wider than the computed widths), and the spans above the threshold as ``{"start", "end", "type", "confidence"}``, both ordered
    by end column.  ONE device->host copy."""
    types, dec, sel = result["types"], result["decoded"], result["selected"]
    B, E = dec["confidence"].shape
    Es = sel["confidence"].shape[1]
    cols = [dec["entities"].reshape(B, E * 3).double(), dec["confidence"].double(), torch.exp(dec["chunk_log_conf"]).double(),
            dec["count"].reshape(B, 1).double(), sel["entities"].reshape(B, Es * 3).double(), sel["confidence"].double(),
            sel["count"].reshape(B, 1).double()]
    packed = torch.cat(cols, dim=1).cpu().numpy()
    out = []
    for row in packed:
        e, c, cc, n, rest = row[:E * 3].reshape(E, 3).astype(np.int64), row[E * 3:E * 4], row[E * 4:E * 5], int(row[E * 5]), \
            row[E * 5 + 1:]
        se, sc, sn = rest[:Es * 3].reshape(Es, 3).astype(np.int64), rest[Es * 3:Es * 4], int(rest[Es * 4])
        out.append({
            "decoded": [{"start": int(e[k, 0]), "end": int(e[k, 1]), "type": types[int(e[k, 2])], "confidence": float(c[k]),
                         "chunk_confidence": float(cc[k])} for k in range(min(n, E))],
            "selected": [{"start": int(se[k, 0]), "end": int(se[k, 1]), "type": types[int(se[k, 2])], "confidence": float(sc[k])}
                         for k in range(min(sn, Es))]})
    return out


def nbest_to_lists(result: dict) -> List[List[Tuple[List[int], float, float]]]:
    """The dict of `CRF.decode_nbest` -> per sentence its ``n_paths`` hypotheses, best first, as ``(tags, score, prob)``:
    the tag list without padding, the unnormalised path score and ``exp(logprob)`` (None if the log-probabilities were not asked
    for).  ONE device->host copy."""
    tags, scores, logprob, n_paths = result["tags"], result["scores"], result["logprob"], result["n_paths"]
    B, K, S = tags.shape
    cols = [tags.reshape(B, K * S).double(), scores.double(), n_paths.reshape(B, 1).double()]
    if logprob is not None:
        cols.append(logprob.double())
    packed = torch.cat(cols, dim=1).cpu().numpy()
    out = []
    for row in packed:
        t, sc, n = row[:K * S].reshape(K, S).astype(np.int64), row[K * S:K * S + K], int(row[K * S + K])
        lp = row[K * S + K + 1:] if logprob is not None else None
        out.append([(t[k][t[k] >= 0].tolist(), float(sc[k]), float(np.exp(lp[k])) if lp is not None else None)
                    for k in range(n)])
    return out


def _prf(correct: int, predicted: int, support: int) -> Tuple[float, float, float]:
    p = correct / predicted if predicted else 0.0
    r = correct / support if support else 0.0
    return p, r, (2 * p * r / (p + r) if p + r else 0.0)


class EntityScorer:
    """Entity-level precision / recall / F1 of decoded tags, counted on the GPU.

    ``update`` adds one batch into a small device counter (one `mtvaf_entity_counts` launch on the current stream, no host
    sync); ``compute`` reads it once.  ``scheme="seqeval"`` counts what ``classification_report`` counts on the
    `label_sequences` lists, ``"reference"`` what modules/eval_metrics.py::evaluate / evaluate_each_class count (see
    `entity_tables`).  ``device=None``: the device of the first ``update``."""

    def __init__(self, label_map: Dict[str, int], scheme: str = "seqeval", skip: Sequence[str] = ("X", "[SEP]"), device=None):
        t = entity_tables(label_map, scheme, skip)
        if t["C"] > 64:
            raise ValueError(f"label ids up to {t['C'] - 1}: the counting kernel reads at most 64 labels (ids 0..63)")
        self.scheme, self.types, self.primary, self.C = scheme, t["types"], t["primary"], t["C"]
        self._tables = [torch.from_numpy(t[k]).reshape(-1) for k in ("start", "end", "type_of", "gold_skip")]
        self.counts = torch.zeros(len(self.types) * 3 + 2, dtype=torch.int64)
        self.device = None
        if device is not None:
            self._place(torch.device(device))

    def _place(self, device):
        self._tables = [x.to(device) for x in self._tables]
        self.counts = self.counts.to(device)
        self.device = device

    def update(self, pred_tags: torch.Tensor, labels: torch.Tensor, attention_mask: torch.Tensor) -> None:
        """pred_tags [B, >=S] int32 on the device as ``CRF.decode_packed`` returns them (-1 beyond each length), labels [B,S],
        attention_mask [B,S] (uint8 is read in place; other dtypes cost a cast)."""
        from . import hip
        if self.device is None:
            self._place(pred_tags.device)
        mask = attention_mask if attention_mask.dtype == torch.uint8 else attention_mask.to(torch.uint8)
        gold = labels if labels.dtype == torch.int64 else labels.to(torch.int64)
        hip.entity_counts(pred_tags, gold.contiguous(), mask.contiguous(), *self._tables, len(self.types), self.counts)

    def reset(self) -> None:
        self.counts.zero_()

    def all_reduce(self, group=None) -> None:
        """Sums the counter over the process group (nothing without one)."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(self.counts, op=dist.ReduceOp.SUM, group=group)

    def compute(self) -> dict:
        """One small device->host copy -> {type: {predicted, support, correct, precision, recall, f1}, ..., "micro": the same
        over all chunks, "macro" / "weighted": {precision, recall, f1, support} over the listed types, "token_accuracy"}.
        Types no B / I / E / S label carries are listed only with non-zero counts; x / 0 reads 0.0."""
        c = self.counts.cpu().tolist()
        out, rows = {}, []
        for t, name in enumerate(self.types):
            predicted, support, correct = c[3 * t:3 * t + 3]
            if self.primary[t] or predicted or support or correct:
                p, r, f = _prf(correct, predicted, support)
                out[name] = dict(predicted=predicted, support=support, correct=correct, precision=p, recall=r, f1=f)
                rows.append(out[name])
        predicted, support, correct = (sum(c[k:3 * len(self.types):3]) for k in range(3))
        p, r, f = _prf(correct, predicted, support)
        result = dict(out)
        result["micro"] = dict(predicted=predicted, support=support, correct=correct, precision=p, recall=r, f1=f)
        n = len(rows)
        result["macro"] = dict(support=support, **{k: (sum(x[k] for x in rows) / n if n else 0.0)
                                                    for k in ("precision", "recall", "f1")})
        result["weighted"] = dict(support=support, **{k: (sum(x[k] * x["support"] for x in rows) / support if support else 0.0)
                                                       for k in ("precision", "recall", "f1")})
        equal, kept = c[-2], c[-1]
        result["token_accuracy"] = equal / kept if kept else 0.0
        return result


# -------------------------------------------------------------------------------------------------
# Calibration of the entity posteriors on the device (csrc/calibration.hip): threshold curves, reliability, ECE, Brier
# -------------------------------------------------------------------------------------------------
def default_log_edges(n_bins: int) -> np.ndarray:
    """fp32 [n_bins + 1]: -inf, log(k / n_bins) for k = 1 .. n_bins - 1, 0 -- equal-width probability bins, stated in log space."""
    e = np.empty(n_bins + 1, dtype=np.float32)
    e[0], e[n_bins] = -np.inf, 0.0
    e[1:n_bins] = np.log(np.arange(1, n_bins, dtype=np.float64) / n_bins).astype(np.float32)
    return e


def _curve(n, hit, gold):
    """n / hit int [NB], gold int -> the threshold curve over the edges k = 0 .. NB-1: the items of the bins >= k are predicted."""
    predicted = np.cumsum(n[::-1])[::-1]
    correct = np.cumsum(hit[::-1])[::-1]
    rows = [_prf(int(c), int(p), int(gold)) for p, c in zip(predicted, correct)]
    return dict(predicted=predicted.tolist(), correct=correct.tolist(), precision=[r[0] for r in rows],
                recall=[r[1] for r in rows], f1=[r[2] for r in rows])


def _reliability(n, hit, sum_p, sum_sq, first_bin):
    """-> (bins table, ece, brier): ece / brier over the bins >= first_bin"""
    with np.errstate(divide="ignore", invalid="ignore"):
        acc = np.where(n > 0, hit / np.maximum(n, 1), 0.0)
        conf = np.where(n > 0, sum_p / np.maximum(n, 1), 0.0)
    total = int(n[first_bin:].sum())
    ece = float((n[first_bin:] / total * np.abs(acc[first_bin:] - conf[first_bin:])).sum()) if total else 0.0
    brier = float(sum_sq[first_bin:].sum() / total) if total else 0.0
    return dict(count=n.tolist(), hits=hit.tolist(), accuracy=acc.tolist(), confidence=conf.tolist()), ece, brier


class CalibrationScorer:
    """Precision / recall over the confidence threshold and the reliability of the tagger's entity posteriors, counted on the GPU.

    An update adds one batch into a small device counter block (`mtvaf_chunk_calibration` / `mtvaf_entity_calibration` on the
    current stream, no host sync); ``compute`` reads it once.  ``update_events`` scores every chunk EVENT of
    `CRF.chunk_posteriors`' ``log_post`` (finite elements only), ``update_entities`` a list of entities with a log confidence
    (`predict`, `predict_constrained`, hypothesis 0 of `predict_nbest`, the ``chunk_log_conf`` / ``selected`` lists of
    `predict_posteriors`).  One instance takes one kind of update: mixing the two raises.  An item is a hit iff the gold labels,
    chunked over the kept columns by the scheme's tables (`entity_tables`), hold that very chunk.

    Bins live in log space: ``edges`` fp32 [n_bins + 1], ascending; the bin of a log-probability lp is the number of k in
    1 .. n_bins-1 with ``lp >= edges[k]``.  The default is `default_log_edges`: log(k / n_bins), the ends -inf and 0.  The array is
    built once on the host, and the kernel reads a copy of the same fp32 values, so host and device agree on every bin.
    ``device=None``: the device of the first update."""

    def __init__(self, label_map: Dict[str, int], scheme: str = "seqeval", skip: Sequence[str] = ("X", "[SEP]"), n_bins: int = 20,
                 edges=None, device=None):
        t = entity_tables(label_map, scheme, skip)
        if t["C"] > 64:
            raise ValueError(f"label ids up to {t['C'] - 1}: the calibration kernels read at most 64 labels (ids 0..63)")
        e = default_log_edges(int(n_bins)) if edges is None else np.asarray(edges, dtype=np.float32).reshape(-1).copy()
        self.n_bins = e.size - 1
        if not 1 <= self.n_bins <= 64:
            raise ValueError(f"{self.n_bins} bins: the calibration kernels read 1 to 64")
        inner = e[1:self.n_bins]
        if np.isnan(e).any() or (np.diff(inner) < 0).any():
            raise ValueError("edges must be ascending log-probabilities without NaN")
        self.scheme, self.types, self.primary, self.C = scheme, t["types"], t["primary"], t["C"]
        self.edges = torch.from_numpy(e)  # the one array of edges: `compute` reads it, the kernels read its device copy
        self._edges_dev = self.edges
        self._tables = [torch.from_numpy(t[k]).reshape(-1) for k in ("start", "end", "type_of")]
        self._skip = torch.from_numpy(t["gold_skip"].astype(bool))
        self._has_skip = bool(t["gold_skip"].any())
        T, NB = len(self.types), self.n_bins
        self.block = torch.zeros(4 * T * NB + 2 * T + 1, dtype=torch.int64)  # layout: include/mtvaf_hip.h
        self.kind = None  # "events" | "entities" after the first update
        self.device = None
        if device is not None:
            self._place(torch.device(device))

    def _place(self, device):
        self._tables = [x.to(device) for x in self._tables]
        self._skip = self._skip.to(device)
        self._edges_dev = self.edges.to(device)
        self.block = self.block.to(device)
        self.device = device

    def _fields(self, block=None):
        """Views of the block -> n, hit [T,NB] int64; gold, gold_reachable [T] int64; sum_p, sum_sq [T,NB] float64; sentences"""
        b = self.block if block is None else block
        T, NB = len(self.types), self.n_bins
        c = T * NB
        return (b[:c].view(T, NB), b[c:2 * c].view(T, NB), b[2 * c:2 * c + T], b[2 * c + T:2 * c + 2 * T],
                b[2 * c + 2 * T:3 * c + 2 * T].view(torch.float64).view(T, NB),
                b[3 * c + 2 * T:4 * c + 2 * T].view(torch.float64).view(T, NB), b[4 * c + 2 * T:])

    def _begin(self, kind, device, labels, attention_mask):
        if self.kind not in (None, kind):
            raise ValueError(f"this CalibrationScorer has taken {self.kind} updates: score {kind} with an instance of their own")
        self.kind = kind
        if self.device is None:
            self._place(device)
        mask = attention_mask if attention_mask.dtype == torch.uint8 else attention_mask.to(torch.uint8)
        gold = labels if labels.dtype == torch.int64 else labels.to(torch.int64)
        return gold.contiguous(), mask.contiguous()

    def update_events(self, log_post: torch.Tensor, keep: torch.Tensor, labels: torch.Tensor, attention_mask: torch.Tensor) -> None:
        """log_post [B,S,W,T] fp32 and keep [B,S] as `CRF.chunk_posteriors` wrote / read them (T = the scheme's types), labels
        [B,S], attention_mask [B,S] (a prefix mask; uint8 is read in place, other dtypes cost a cast)."""
        from . import hip
        if log_post.dim() != 4 or log_post.shape[3] != len(self.types):
            raise ValueError(f"log_post {tuple(log_post.shape)}: expected [B, S, W, {len(self.types)}] for the types {self.types}")
        gold, mask = self._begin("events", log_post.device, labels, attention_mask)
        keep = None if keep is None else keep.to(torch.uint8).contiguous()
        hip.chunk_calibration(log_post.detach().contiguous(), gold, mask, keep, *self._tables, self._edges_dev, self.block)

    def update_entities(self, entities: torch.Tensor, log_confidence: torch.Tensor, labels: torch.Tensor,
                        attention_mask: torch.Tensor, keep=None) -> None:
        """entities [B,E,3] int32 (start column, end column, type index; -1 in unused slots) and log_confidence [B,E] fp32 in
        `CRF.entities`' format, labels [B,S], attention_mask [B,S].  ``keep`` [B,S]: the columns the gold labels are chunked
        over; None: columns 1 .. L-1 minus those whose gold label is one of ``skip`` -- `EntityScorer`'s columns."""
        from . import hip
        gold, mask = self._begin("entities", entities.device, labels, attention_mask)
        if keep is None:
            if self._has_skip:
                g = torch.where((gold >= 0) & (gold < self.C), gold, torch.zeros_like(gold))
                keep = torch.cumprod(mask, dim=1).bool() & ~self._skip[g]
                keep[:, 0] = False
                keep = keep.to(torch.uint8)
        else:
            keep = keep.to(torch.uint8).contiguous()
        ents = entities if entities.dtype == torch.int32 else entities.to(torch.int32)
        hip.entity_calibration(ents.contiguous(), log_confidence.detach().to(torch.float32).contiguous(), gold, mask, keep,
                               *self._tables, self._edges_dev, len(self.types), self.block)

    def reset(self) -> None:
        self.block.zero_()

    def all_reduce(self, group=None) -> None:
        """Sums the block over the process group (nothing without one): the integer fields as integers, the two sums as float64."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            ints_end = 2 * len(self.types) * (self.n_bins + 1)  # n, hit, gold, gold_reachable: one contiguous run
            f64 = self.block[ints_end:-1].view(torch.float64)    # sum_p, sum_sq: the next
            for part in (self.block[:ints_end], f64, self.block[-1:]):
                dist.all_reduce(part, op=dist.ReduceOp.SUM, group=group)

    def compute(self, first_bin: int = 1) -> dict:
        """One small device->host copy -> a dict:

        ``edges`` (log) and ``thresholds`` = exp(edges) [n_bins + 1]; per listed type under ``types[name]`` and over all types
        under ``pooled``: ``bins`` = {count, hits, accuracy = hits / count, confidence = sum p / count} per bin, ``curve`` =
        {predicted, correct, precision, recall, f1} per edge k = 0 .. n_bins-1, where the items of the bins >= k are the
        predictions (``predicted[k]`` = sum of count over j >= k, ``correct[k]`` the same over hits; precision = correct /
        predicted, recall = correct / gold), plus gold, gold_reachable, recall_ceiling, ece, brier.  ``micro`` is the pooled
        curve.  ``best_f1`` / ``best_k`` / ``best_threshold``: the greatest micro F1, the LOWEST k that reaches it, and
        ``exp(edges[k])`` (0.0 for k = 0: everything is predicted).  ``recall_ceiling`` = gold_reachable / gold: the recall no
        threshold can exceed, below 1 when gold chunks are wider than the computed widths.  ``sentences``, ``kind``.

        ``ece`` = sum_k (n_k / N) |accuracy_k - confidence_k| and ``brier`` = sum (p - y)^2 / N run over the bins >=
        ``first_bin``, N their items.  The default ``first_bin=1`` leaves bin 0 out: among the dense events it holds the
        near-impossible ones -- almost every span of a sentence -- whose |0 - p| ~ 0 would drown both figures; ``first_bin=0``
        takes every scored item.  Types no B / I / E / S label carries are listed only with non-zero counts; x / 0 reads 0.0."""
        if not 0 <= first_bin <= self.n_bins:
            raise ValueError(f"first_bin={first_bin} outside 0..{self.n_bins}")
        n, hit, gold, reach, sum_p, sum_sq, sentences = (x.numpy() for x in self._fields(self.block.cpu()))
        edges = self.edges.numpy()
        with np.errstate(over="ignore"):
            thresholds = np.exp(edges.astype(np.float64))

        def section(rows):
            nn, hh, sp, sq = (x[rows].sum(axis=0) for x in (n, hit, sum_p, sum_sq))
            g, r = int(gold[rows].sum()), int(reach[rows].sum())
            bins, ece, brier = _reliability(nn, hh, sp, sq, first_bin)
            return dict(bins=bins, curve=_curve(nn, hh, g), gold=g, gold_reachable=r, recall_ceiling=r / g if g else 0.0, ece=ece,
                        brier=brier)
        out = {"edges": edges.tolist(), "thresholds": thresholds.tolist(), "types": {}}
        for t, name in enumerate(self.types):
            if self.primary[t] or n[t].any() or gold[t]:
                out["types"][name] = section([t])
        pooled = section(list(range(len(self.types))))
        f1 = pooled["curve"]["f1"]
        best = max(range(self.n_bins), key=lambda k: (f1[k], -k))  # the lowest k among ties
        out.update(pooled=pooled, micro=pooled["curve"], best_k=best, best_f1=f1[best], best_threshold=float(thresholds[best]),
                   ece=pooled["ece"], brier=pooled["brier"], recall_ceiling=pooled["recall_ceiling"], sentences=int(sentences[0]),
                   kind=self.kind, first_bin=first_bin)
        return out


def calibration_to_rows(result: dict) -> List[dict]:
    """The dict of `CalibrationScorer.compute` -> plain rows for printing: one ``{"table": "bins", "type", "bin", "low", "high",
    "count", "hits", "accuracy", "confidence"}`` per type (and "pooled") and bin, ``low`` / ``high`` the bin's probability range;
    then one ``{"table": "curve", "type", "k", "threshold", "predicted", "correct", "precision", "recall", "f1"}`` per type (and
    "micro") and edge."""
    th = result["thresholds"]
    sections = list(result["types"].items()) + [("pooled", result["pooled"])]
    rows = []
    for name, sec in sections:
        b = sec["bins"]
        for k in range(len(b["count"])):
            rows.append(dict(table="bins", type=name, bin=k, low=th[k], high=th[k + 1], count=b["count"][k], hits=b["hits"][k],
                             accuracy=b["accuracy"][k], confidence=b["confidence"][k]))
    for name, sec in sections:
        c = sec["curve"]
        for k in range(len(c["predicted"])):
            rows.append(dict(table="curve", type="micro" if name == "pooled" else name, k=k, threshold=th[k],
                             predicted=c["predicted"][k], correct=c["correct"][k], precision=c["precision"][k],
                             recall=c["recall"][k], f1=c["f1"][k]))
    return rows


# -------------------------------------------------------------------------------------------------
# Aspect-level score of the span model on the device (csrc/span_score.hip): eval_absa's counts
# -------------------------------------------------------------------------------------------------
SPAN_CLASSES = ("other", "neutral", "positive", "negative")  # models/utils.py:17 id_to_label, the classifier's four outputs


class SpanScorer:
    """Precision / recall / F1 of `TVNetSAModel.predict`'s aspect terms against the gold terms, counted on the GPU: what
    modules/eval_metrics.py::eval_absa counts after the trainer's per-sentence host copies (modules/train.py:200-209).

    ``update`` adds one batch into a small device counter (one `mtvaf_span_counts` launch on the current stream, no host
    sync); ``compute`` reads it once.  ``classes`` names the class ids; ``len(classes)`` must equal the K of the logits.
    Terms are compared by word-key signature and class (include/mtvaf_hip.h), not by normalised text.  ``device=None``: the
    device of the first ``update``."""

    def __init__(self, classes: Sequence[str] = SPAN_CLASSES, device=None):
        self.classes = tuple(classes)
        if not 2 <= len(self.classes) <= 8:
            raise ValueError(f"{len(self.classes)} classes: the counting kernel reads 2 to 8")
        self.counts = torch.zeros(3 * len(self.classes) + 2, dtype=torch.int64)
        self.device = None
        if device is not None:
            self._place(torch.device(device))

    def _place(self, device):
        self.counts = self.counts.to(device)
        self.device = device

    def update(self, pred: dict, gold_starts, gold_ends, gold_class, gold_masks, word_index, word_key=None, return_slots=False):
        """pred: the dict of `TVNetSAModel.predict` (span_starts, span_ends, label_masks [B,N], logits [B,N,K]); gold_* [B,G]:
        the feature's start_indexes, end_indexes, polarity_labels, label_masks; word_index [B,S] token -> word (-1 outside the
        word map), word_key [B,S] or None (= word_index).  int64 / int32 / fp32 contiguous tensors are read in place, others
        cost a cast.  -> None, or with ``return_slots`` (pred_class, matched_gold) [B,N] int32: the class of every slot (-1:
        no such slot) and the lowest gold slot it matches (-1: none)."""
        from . import hip
        logits = pred["logits"]
        if logits.dim() != 3 or logits.shape[2] != len(self.classes):
            raise ValueError(f"logits {tuple(logits.shape)}: expected [B, N, {len(self.classes)}] for classes {self.classes}")
        dev = logits.device
        if self.device is None:
            self._place(dev)

        def as_(t, dtype):
            return t.detach().to(device=dev, dtype=dtype).contiguous()
        spans = [as_(pred[k], torch.int64) for k in ("span_starts", "span_ends", "label_masks")]
        gold = [as_(t, torch.int64) for t in (gold_starts, gold_ends, gold_class, gold_masks)]
        slots = [torch.empty(logits.shape[:2], dtype=torch.int32, device=dev) for _ in range(2)] if return_slots else [None, None]
        hip.span_counts(*spans, as_(logits, torch.float32), *gold, as_(word_index, torch.int32),
                        None if word_key is None else as_(word_key, torch.int32), self.counts, *slots)
        return tuple(slots) if return_slots else None

    def reset(self) -> None:
        self.counts.zero_()

    def all_reduce(self, group=None) -> None:
        """Sums the counter over the process group (nothing without one)."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(self.counts, op=dist.ReduceOp.SUM, group=group)

    def compute(self) -> dict:
        """One small device->host copy -> {class: {retrieved, relevant, common, precision, recall, f1}, ..., "micro": eval_absa's
        {p, r, f1, common, retrieved, relevant} over all terms (``relevant`` includes the gold terms of a class outside the
        list), "macro": {precision, recall, f1} over the classes with a non-zero count, "sentences"}.  x / 0 reads 0.0
        (eval_absa divides by ``relevant`` unguarded: it raises on a set without gold terms)."""
        c = self.counts.cpu().tolist()
        K = len(self.classes)
        out, rows = {}, []
        for k, name in enumerate(self.classes):
            retrieved, relevant, common = c[3 * k:3 * k + 3]
            p, r, f = _prf(common, retrieved, relevant)
            out[name] = dict(retrieved=retrieved, relevant=relevant, common=common, precision=p, recall=r, f1=f)
            if retrieved or relevant or common:
                rows.append(out[name])
        retrieved, relevant, common = (sum(c[j:3 * K:3]) for j in range(3))
        relevant += c[3 * K]
        p, r, f = _prf(common, retrieved, relevant)
        out["micro"] = dict(p=p, r=r, f1=f, common=common, retrieved=retrieved, relevant=relevant)
        n = len(rows)
        out["macro"] = {k: (sum(x[k] for x in rows) / n if n else 0.0) for k in ("precision", "recall", "f1")}
        out["sentences"] = c[3 * K + 1]
        return out
