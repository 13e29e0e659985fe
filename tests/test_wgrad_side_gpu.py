"""Backward-weight on the side stream (wgrad_side.py): what the scratch buffer of a side-stream launch belongs to, and
that the bf16 convolution's gradients do not depend on the schedule."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _segment_stream(t: torch.Tensor) -> int:
    """The stream the caching allocator booked the segment holding `t` to."""
    p = t.data_ptr()
    for seg in torch.cuda.memory_snapshot():
        if seg["address"] <= p < seg["address"] + seg["total_size"]:
            return seg["stream"]
    raise AssertionError("tensor not found in the allocator's segments")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_grown_side_stream_scratch_belongs_to_the_side_stream(dtype, monkeypatch):
    """Backward-weight into `.grad` storage uses the side stream's scratch buffer (ops.workspace).  A larger shape grows
    it and drops the old one: unless the caching allocator books the buffer to the side stream, the dropped block can
    go at once to a main-stream allocation while the lagging side stream is still writing partial sums into it."""
    from unlearn_saliency_amd import conv_bf16, ops, wgrad_side
    from unlearn_saliency_amd.conv import use_salun_convs
    from unlearn_saliency_amd.flat import arena_of
    monkeypatch.setattr(wgrad_side, "OVERLAP", True)
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Conv2d(32, 32, 3, padding=1)).cuda()
    assert (use_salun_convs(model) if dtype == "fp32" else conv_bf16.use_salun_convs_bf16(model)) == 1
    arena = arena_of(model)  # .grad views of the flat gradient: the sink path, which launches beside
    dev = torch.device("cuda", torch.cuda.current_device())
    side = wgrad_side.stream(dev)
    key = (dev.index, side.cuda_stream, "")
    torch.cuda.synchronize()
    ops._ws.pop(key, None)  # start from no buffer, whatever earlier tests left
    sizes = []
    for n, hw in ((2, 8), (8, 64)):  # 0.1 MB, then 9.4 MB (fp32) / 2.4 MB (bf16) of backward-weight scratch
        x = torch.randn(n, 32, hw, hw, device="cuda")
        if dtype == "bf16":
            x = x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        arena.zero_grad()
        model(x).float().square().mean().backward()
        torch.cuda.synchronize()
        ws = ops._ws[key]
        sizes.append(ws.numel())
        assert _segment_stream(ws) == side.cuda_stream, (n, hw)
    assert sizes[1] > sizes[0], sizes
    assert float(model[0].weight.grad.abs().max()) > 0


@pytest.mark.parametrize("R", [3, 1])
def test_bf16_side_stream_changes_no_gradient_bit(R, monkeypatch):
    """SalunConv2dBF16 with its gradients in the flat arena: with backward-weight on the side stream, weight.grad and the
    gradient of the `nbias` term equal the one-stream result bit for bit, run after run.  bias.grad takes another
    summation order there: on one stream the kernel that also gives the per-image sums of the `nbias` gradient sums the
    bias per image; beside, those sums are a launch of their own and the bias is the plain column sum.  It equals, bit for
    bit, what one stream gives when no `nbias` gradient is asked for."""
    from unlearn_saliency_amd import conv_bf16, wgrad_side
    from unlearn_saliency_amd.flat import arena_of
    torch.manual_seed(7)
    model = torch.nn.Sequential(torch.nn.Conv2d(64, 96, R, padding=R // 2)).cuda()
    assert conv_bf16.use_salun_convs_bf16(model) == 1
    conv = model[0]
    arena = arena_of(model)
    x = torch.randn(4, 64, 16, 16, device="cuda").to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    emb = torch.randn(4, 96, device="cuda")
    dy = torch.randn(4, 96, 16, 16, device="cuda").to(torch.bfloat16)

    def grads(overlap, want_nbias=True):
        monkeypatch.setattr(wgrad_side, "OVERLAP", overlap)
        arena.zero_grad()
        e = emb.clone().requires_grad_(want_nbias)
        conv(x, nbias=e).backward(dy)
        torch.cuda.synchronize()
        return conv.weight.grad.clone(), conv.bias.grad.clone(), e.grad

    w_ref, b_ref, nb_ref = grads(False)
    w_plain, b_plain, _ = grads(False, want_nbias=False)
    assert torch.equal(w_plain, w_ref) and float(w_ref.abs().max()) > 0 and float(nb_ref.abs().max()) > 0
    for _ in range(3):
        w, b, nb = grads(True)
        assert torch.equal(w, w_ref)
        assert torch.equal(nb, nb_ref)
        assert torch.equal(b, b_plain)
        assert float((b - b_ref).abs().max()) <= 1e-5 * float(b_ref.abs().max())
