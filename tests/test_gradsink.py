"""Engine behaviour that gradsink.py relies on (CPU): a leaf whose custom Function returns None for its gradient
still gets its post-accumulate-grad hooks fired exactly once per backward, and sink() declines whenever writing
into .grad directly would not be equivalent to autograd's own accumulation.  On the device: the pair rule of gamma /
beta with a hook on one member, and the destination of a parameter that has no `.grad` yet."""
import pytest
import torch

from unlearn_saliency_amd import gradsink


class _Mul(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        return x * w

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        if w.grad is not None:  # what the HIP kernels do: add into the existing storage, hand autograd nothing
            w.grad.add_(g * x)
            return g * w, None
        return g * w, g * x


def test_post_accumulate_hooks_fire_once_even_when_function_returns_none():
    w = torch.nn.Parameter(torch.full((3,), 2.0))
    x = torch.ones(3, requires_grad=True)
    fired = []
    w.register_post_accumulate_grad_hook(lambda p: fired.append(p.grad.clone()))
    _Mul.apply(x, w).sum().backward()  # first: autograd route (no .grad yet)
    _Mul.apply(x, w).sum().backward()  # second: direct accumulation, None returned
    assert len(fired) == 2
    assert torch.equal(fired[0], torch.ones(3)) and torch.equal(fired[1], torch.full((3,), 2.0))


def test_sink_declines_when_not_equivalent():
    p = torch.nn.Parameter(torch.zeros(4))
    with torch.no_grad():
        assert gradsink.sink(p) is None  # no .grad
        p.grad = torch.zeros(4)
        assert gradsink.sink(p) is None  # host tensor: the kernels only write device memory
        assert gradsink.sink(None) is None and gradsink.sink(torch.zeros(4)) is None
    assert gradsink.sink(p) is None  # grad mode on (double backward)


@pytest.mark.gpu
def test_pair_sinks_both_or_neither_and_single_form_allocates():
    """gamma / beta go into `.grad` together or not at all (their kernels have one accumulate switch): a tensor hook on
    ONE of them sends both back to autograd, in the kernel-allocates flavour and in the caller-allocates one."""
    def shares_storage(a, b):
        return a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()

    g = torch.nn.Parameter(torch.ones(6, device="cuda"))
    b = torch.nn.Parameter(torch.zeros(6, device="cuda"))
    g.grad, b.grad = torch.zeros_like(g), torch.zeros_like(b)
    bare = torch.nn.Parameter(torch.ones(3, 5, device="cuda"))
    with torch.no_grad():
        for fresh in (None, torch.empty):
            dg, db = gradsink.pair(g, b, fresh)
            assert dg.out is g.grad and db.out is b.grad
            assert dg.accumulate is True and db.accumulate is True
            assert dg.returned(torch.ones(6)) is None and db.returned() is None
        b.register_hook(lambda grad: grad)
        dg, db = gradsink.pair(g, b)  # the kernel allocates
        assert dg.out is None and db.out is None
        assert dg.accumulate is False and db.accumulate is False
        made_g, made_b = torch.ones(6, device="cuda"), torch.ones(6, device="cuda")
        assert dg.returned(made_g) is made_g and db.returned(made_b) is made_b
        dg, db = gradsink.pair(g, b, torch.empty)  # the caller allocates
        for d, p in ((dg, g), (db, b)):
            assert d.out.shape == p.shape and d.out.dtype == torch.float32 and d.out.is_cuda
            assert not shares_storage(d.out, g.grad) and not shares_storage(d.out, b.grad)
            assert d.accumulate is False
            assert d.returned() is d.out
        assert not shares_storage(dg.out, db.out)
        d = gradsink.dest(bare, torch.zeros)  # no .grad yet
        assert d.accumulate is False and d.out.shape == bare.shape and d.out.is_cuda
        assert torch.equal(d.out, torch.zeros_like(bare))
        assert d.returned() is d.out
