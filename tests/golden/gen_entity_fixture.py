"""Entity-chunk fixture: drives the REAL reference `modules/eval_metrics.py::get_chunks / evaluate / evaluate_each_class` (imported
from the reference checkout in the authoring container through the shim of gen_golden.py) on random label-id batches and records
the inputs and the integer counts behind the reference's ratios:

    python tests/golden/gen_entity_fixture.py        # writes tests/golden/entity_chunks.npz

Per label set s ("a": the trainer's ten labels numbered from 1 plus PAD = 0; "b": the 16 BIOES labels of modules/dataset.py:65
numbered from 0):
    {s}_gold [B,S] int64   {s}_pred [B,S] int32   {s}_mask [B,S] uint8
    {s}_types [T] str      {s}_counts [T,3] int64 = predicted, gold, correct chunks per type   {s}_tokens [2] = equal, kept
The kept label-id lists are built here as the trainer's loop builds its name lists (modules/train.py:627-647: from column 1 while
the mask is 1, gold X / [SEP] dropped) and handed to the reference as ids with its label map as `tags`.  The counts come from the
sets get_chunks returns; `evaluate` and `evaluate_each_class` return ratios, and the generator ASSERTS that every ratio they
return is the ratio of the stored counts.  Numbers and type names only: nothing of the reference's text is stored.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

import gen_golden as G  # noqa: E402

B, S = 40, 48


def kept_ids(gold, pred, mask, skip_ids):
    y_true, y_pred = [], []
    for b in range(gold.shape[0]):
        gs, ps = [], []
        for c in range(1, gold.shape[1]):
            if not mask[b, c]:
                break
            if int(gold[b, c]) not in skip_ids:
                gs.append(int(gold[b, c]))
                ps.append(int(pred[b, c]))
        y_true.append(gs)
        y_pred.append(ps)
    return y_true, y_pred


def ratio(correct, total):
    return correct / total if correct > 0 else 0


def main():
    G.install_shim()
    import modules.eval_metrics as EM
    import entity_cases as E

    rng = np.random.default_rng(20241018)
    out = {}
    for s in ("a", "b"):
        lmap = E.label_map(s)
        tags = dict(lmap)
        if 0 not in tags.values():
            tags["PAD"] = 0  # the trainer's label_map[0] = "PAD" (modules/train.py:628)
        gold, pred, mask = E.make_case(rng, lmap, B, S, mask_kind="ragged", pred_kind="mixed", skip_density=0.25)
        mask[3, 5], mask[7, 2] = 0, 0  # holes: the loop stops there
        pred = np.where(mask.astype(bool), pred, -1).astype(np.int32)
        pred[:B // 4] = np.where(mask[:B // 4].astype(bool), gold[:B // 4], -1)  # some sentences fully right
        y_true, y_pred = kept_ids(gold, pred, mask, {tags[n] for n in E.SKIP if n in tags})
        assert all(0 <= t < len(tags) for row in y_pred for t in row)

        idx_to_tag = {i: n for n, i in tags.items()}
        types = sorted({EM.get_chunk_type(i, idx_to_tag)[1] for i in idx_to_tag if i != tags["O"]})
        counts = np.zeros((len(types), 3), dtype=np.int64)
        for lab, lab_pred in zip(y_true, y_pred):
            gc, pc = EM.get_chunks(lab, tags), EM.get_chunks(lab_pred, tags)
            assert len(set(gc)) == len(gc) and len(set(pc)) == len(pc)
            for k, t in enumerate(types):
                mine = {c for c in pc if c[0] == t}
                counts[k] += (len(mine), len({c for c in gc if c[0] == t}), len(mine & set(gc)))
        equal = sum(a == b for lab, lab_pred in zip(y_true, y_pred) for a, b in zip(lab, lab_pred))
        kept = sum(len(lab) for lab in y_true)

        # the reference's own ratios are the ratios of these counts
        acc, f1, p, r = EM.evaluate(y_pred, y_true, tags)
        tp, tg, tc = (int(v) for v in counts.sum(0))
        assert (p, r) == (ratio(tc, tp), ratio(tc, tg)) and acc == equal / kept, (p, r, acc)
        assert f1 == (2 * p * r / (p + r) if tc > 0 else 0)
        for k, t in enumerate(types):
            f1, p, r = EM.evaluate_each_class(y_pred, y_true, tags, t)
            cp, cg, cc = (int(v) for v in counts[k])
            assert (p, r) == (ratio(cc, cp), ratio(cc, cg)), (t, p, r, counts[k])
        out.update({f"{s}_gold": gold, f"{s}_pred": pred, f"{s}_mask": mask, f"{s}_types": np.array(types),
                    f"{s}_counts": counts, f"{s}_tokens": np.array([equal, kept], dtype=np.int64)})
        print(f"set {s}: kept {kept}, equal {equal}; predicted / gold / correct per type:",
              {t: counts[k].tolist() for k, t in enumerate(types) if counts[k].any()})
    path = os.path.join(HERE, "entity_chunks.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
