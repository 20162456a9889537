"""Gradient clipping inside the AdamW step, host side: the float64 restatement the GPU tests measure against is
torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW, the library exports the new entry points, and the two configurations that
cannot clip refuse."""
import types

import pytest
import torch

import gradclip_cases as GC

NEW_SYMBOLS = ["mtvaf_grad_sqnorm_multi", "mtvaf_grad_sqnorm_workspace_bytes", "mtvaf_grad_clip_finalize", "mtvaf_adamw_dev",
               "mtvaf_adamw_planes_dev", "mtvaf_adamw_multi_dev"]


def test_float64_restatement_is_torch_clip_grad_norm_then_torch_adamw():
    g = torch.Generator().manual_seed(1)
    shapes = [(7,), (5, 3), (1,), (4, 4), (33,)]
    init = [torch.randn(s, generator=g, dtype=torch.float64) for s in shapes]
    grads = [torch.randn(s, generator=g, dtype=torch.float64) for s in shapes]
    grads[2] = None  # a parameter without a gradient: left out of the norm and of the update
    hyper = [dict(lr=3e-3, weight_decay=1e-2), dict(lr=5e-2, weight_decay=1e-2)]
    max_norm = GC.CLIP_FRACTION * GC.global_norm([x for x in grads if x is not None])
    tp = [torch.nn.Parameter(t.clone()) for t in init]
    topt = torch.optim.AdamW([dict(params=tp[:3], **hyper[0]), dict(params=tp[3:], **hyper[1])], betas=(GC.BETA1, GC.BETA2), eps=GC.EPS)
    rp = [t.clone() for t in init]
    ref = GC.ClipAdamW64([dict(params=rp[:3], **hyper[0]), dict(params=rp[3:], **hyper[1])], max_norm)
    clipped = []
    for scale in GC.STEP_SCALES:
        for p, x in zip(tp, grads):
            p.grad = None if x is None else (x * scale).clone()
        tn = torch.nn.utils.clip_grad_norm_(tp, max_norm)
        topt.step()
        norm, coef = ref.step([None if x is None else x * scale for x in grads])
        assert abs(norm - float(tn)) <= 1e-12 * norm
        clipped.append(coef < 1.0)
        for p, q in zip(tp, rp):
            torch.testing.assert_close(q, p.detach(), rtol=1e-12, atol=0)
    assert clipped == [True, True, False]
    assert torch.equal(rp[2], init[2])


def test_restatement_without_a_bound_is_plain_adamw_and_reports_the_norm():
    p = [torch.ones(3, dtype=torch.float64)]
    ref = GC.ClipAdamW64([dict(params=p, lr=1e-3, weight_decay=0.0)], 0.0)
    norm, coef = ref.step([torch.tensor([3.0, 4.0, 0.0])])
    assert norm == 5.0 and coef == 1.0
    assert GC.clip_coef(8.0, 2.0) == 2.0 / (8.0 + 1e-6) and GC.clip_coef(1.0, 2.0) == 1.0


def test_norm_case_list_covers_the_paths_of_the_kernel():
    ts = GC.norm_tensors()
    assert len(ts) > 48  # more than one launch table
    assert any(t.numel() == GC.CHUNK for t in ts) and any(t.numel() == GC.CHUNK + 1 for t in ts)
    assert any(t.storage_offset() == 1 and t.numel() > GC.CHUNK for t in ts)  # unaligned, and the scalar body crosses a chunk
    assert GC.expected_slots([GC.CHUNK, GC.CHUNK + 1, 3 * GC.CHUNK + 5, 1]) == 1 + 2 + 4 + 1


def test_library_exports_the_gradient_clipping_entry_points():
    from mtvaf_amd import hip
    assert set(NEW_SYMBOLS) <= set(hip.exported_symbols())
    hip.lib()  # binds them: raises if the built library lacks one


def test_workspace_query_counts_one_double_per_chunk():
    """Host logic of the library: no GPU call."""
    import ctypes
    from mtvaf_amd import hip
    lengths = [1, GC.CHUNK, GC.CHUNK + 1, 3 * GC.CHUNK + 5]
    arr = (ctypes.c_long * len(lengths))(*lengths)
    assert hip.lib().mtvaf_grad_sqnorm_workspace_bytes(len(lengths), arr) == 8 * GC.expected_slots(lengths)
    assert hip.lib().mtvaf_grad_sqnorm_workspace_bytes(0, None) == 0
    bad = (ctypes.c_long * 2)(5, 0)
    assert hip.lib().mtvaf_grad_sqnorm_workspace_bytes(2, bad) == 0


def test_overlap_with_clipping_raises_at_construction():
    from mtvaf_amd.optim import AdamW
    p = [torch.nn.Parameter(torch.zeros(4))]
    with pytest.raises(ValueError, match="overlap=False"):
        AdamW(p, lr=1e-3, overlap=True, max_grad_norm=1.0)
    with pytest.raises(ValueError, match="overlap=False"):
        AdamW(p, lr=1e-3, overlap=True, track_grad_norm=True)
    with pytest.raises(ValueError):
        AdamW(p, lr=1e-3, max_grad_norm=-1.0)
    opt = AdamW(p, lr=1e-3, max_grad_norm=1.0)  # and without overlap it constructs, with nothing allocated yet
    assert opt.max_grad_norm == 1.0 and opt.skip_nonfinite and opt.last_grad_norm is None and opt.skipped_steps is None
    assert AdamW(p, lr=1e-3).max_grad_norm == 0.0


def test_build_optimizer_on_a_cpu_model_refuses_to_ignore_max_grad_norm():
    from mtvaf_amd.optim import build_optimizer
    model = torch.nn.Linear(4, 3)
    args = types.SimpleNamespace(lr=1e-3, warmup_ratio=0.0, use_prefix=False, max_grad_norm=1.0)
    with pytest.raises(ValueError, match="max_grad_norm"):
        build_optimizer(model, args, 10)
    args.max_grad_norm = 0.0
    opt, _ = build_optimizer(model, args, 10)
    assert isinstance(opt, torch.optim.AdamW)
