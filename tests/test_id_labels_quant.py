"""``sigmoid_contrastive_loss_ids(quant=)`` without a GPU."""

import pytest
import torch

from distributed_sigmoid_loss_amd import sigmoid_contrastive_loss_ids


def _run(quant):
    g = torch.Generator().manual_seed(0)
    zi, zt = (torch.randn(r, 8, generator=g, requires_grad=True)
              for r in (9, 7))
    tp, bias = (torch.tensor(v, requires_grad=True) for v in (1.0, -0.5))
    img, txt = (torch.randint(-1, 3, (r,), generator=g) for r in (9, 7))
    loss = sigmoid_contrastive_loss_ids(zi, zt, tp, bias, img, txt,
                                        impl="torch", quant=quant)
    loss.backward()
    return loss.detach(), zi.grad, zt.grad, tp.grad, bias.grad


@pytest.mark.parametrize("quant", ["fp8", "int8"])
def test_unbuilt_and_unknown_quant_raise(quant):
    with pytest.raises(ValueError, match="quant"):
        _run(quant)


def test_torch_path_ignores_mixed():
    assert all(map(torch.equal, _run("mixed"), _run("bf16")))
