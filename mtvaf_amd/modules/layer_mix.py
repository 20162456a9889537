"""Layer mix: a learned weighted sum of the encoder's hidden states for the heads (ELMo's scalar mix; new functionality, the
reference's heads read the last layer only).  DESIGN.md section 4.26.

    y = gamma * sum_j softmax(scalars)_j * h_{k_j}

over the chosen states k_0 < ... < k_{K-1} of (embedding output, layer 1, ..., layer L).  The module only holds the two
parameters and the selection: the arithmetic runs inside the encoder's autograd node (`engine.EncoderMixFunction`,
csrc/layermix.hip), which `BertModel(..., layer_mix=module)` selects."""
from __future__ import annotations

import torch
from torch import nn

from .. import engine


class LayerMix(nn.Module):
    """``num_states``: L + 1, the embedding output and every layer's output.  ``layers``: ``"all"`` or a list of state indices
    (0 = embedding output, l = layer l, negative ones count from the end; at most 32, each once).  ``init_last`` is added to the
    last chosen state's scalar, so that a run can start near "last layer only" (softmax weight e^x / (e^x + K - 1)).

    Parameters: ``scalars`` [K] fp32, zeros; ``gamma`` [1] fp32, one.  Both belong in the optimizer's no-decay group
    (`optim.finetune_param_groups` puts them there)."""

    def __init__(self, num_states: int, layers="all", init_last: float = 0.0):
        super().__init__()
        self.num_states = int(num_states)
        self.layers = engine.resolve_mix_layers(layers, self.num_states)
        scalars = torch.zeros(len(self.layers), dtype=torch.float32)
        scalars[-1] += float(init_last)
        self.scalars = nn.Parameter(scalars)
        self.gamma = nn.Parameter(torch.ones(1, dtype=torch.float32))

    def weights(self) -> torch.Tensor:
        """softmax(scalars) [K] on the parameter's device, detached (no host read)."""
        return torch.softmax(self.scalars.detach().float(), dim=0)

    def extra_repr(self) -> str:
        return f"num_states={self.num_states}, layers={list(self.layers)}"
