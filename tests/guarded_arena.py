"""The guarded device arena of the exact-answer GPU tests (test_conv_exact_gpu.py, test_gemm_exact_gpu.py,
test_conv_bf16_exact_gpu.py): every tensor of a call lies 16-byte aligned in ONE flat allocation with GUARD floats of NaN
before and after every input and of a sentinel pattern around every output (and in the output itself before the call);
after the call everything but the outputs must hold the bits it was given.  A part is fp32 (4-byte words) or, with
dtype="bf16", bf16 (two elements per word; an OUTPUT without initial data may hold an odd number of them: the upper half of
its last word is guard, checked like one); guards, alignment and skew are in words either way."""
from ctypes import c_void_p

import torch

GUARD = 4096
NAN_BITS, SENTINEL = 0x7FC00000, 0x7FA5A5A5      # a quiet NaN; a NaN pattern no computation produces


def _bf16_words(data):
    """bf16 data (a float tensor, rounded to bf16, or int16 bit patterns) as the int32 words that hold it."""
    flat = data.reshape(-1)
    if flat.dtype != torch.int16:
        flat = flat.float().bfloat16().view(torch.int16)
    return flat.contiguous().view(torch.int32)


class Arena:
    """The tensors of one call inside one flat device allocation, each behind and before GUARD floats."""

    def __init__(self):
        self.parts, self.fills, self.n, self.bf16, self.odd = {}, [], 0, set(), {}

    def put(self, name, data=None, shape=None, out=False, skew=0, dtype="f32"):
        """An input (data given), an output (shape given; filled with the sentinel) or an in-place output (both).
        skew: floats off the 16-byte boundary.  dtype "bf16": 2-byte elements (parts[name] counts its 4-byte words)."""
        shape = tuple(data.shape) if data is not None else tuple(shape)
        numel = 1
        for s in shape:
            numel *= s
        assert dtype in ("f32", "bf16")
        if dtype == "bf16":
            if numel % 2:
                assert out and data is None, "only an output filled with the sentinel may end inside a word"
                self.odd[name] = numel
            numel = (numel + 1) // 2
            self.bf16.add(name)
            data = None if data is None else _bf16_words(data)
        start = self.n + GUARD + skew
        end = (start + numel + 3) // 4 * 4
        self.fills.append((self.n, end + GUARD, SENTINEL if out else NAN_BITS, start, data))
        self.parts[name] = (start, numel, shape, out)
        self.n = end + GUARD
        return self

    def upload(self):
        host = torch.empty(self.n, dtype=torch.int32)
        for lo, hi, bits, start, data in self.fills:
            host[lo:hi] = bits
            if data is not None:
                flat = data.reshape(-1)            # int32 data is a bit pattern (an output with sentinels inside it)
                host[start:start + data.numel()] = flat if flat.dtype == torch.int32 else flat.float().view(torch.int32)
        self.host, self.dev = host, host.cuda()
        return self

    def ptr(self, name):
        return c_void_p(self.dev.data_ptr() + 4 * self.parts[name][0]) if name in self.parts else c_void_p(None)

    def download(self):
        """The whole arena on the host (int32 bit patterns), after checking that nothing outside the outputs changed."""
        torch.cuda.synchronize()
        after = self.dev.cpu()
        lo = 0
        for start, numel, _, out in sorted(self.parts.values()) + [(self.n, 0, None, True)]:
            if out:                                # everything between two outputs: inputs and all the guards
                assert torch.equal(after[lo:start], self.host[lo:start]), "a guard or an input was written"
                lo = start + numel
        for name in self.odd:                      # the half word behind an odd-sized bf16 output
            last = self.parts[name][0] + self.parts[name][1] - 1
            assert after[last:last + 1].view(torch.int16)[1] == self.host[last:last + 1].view(torch.int16)[1], "a guard was written"
        return after

    def part(self, after, name):
        """The output `name` of a downloaded arena."""
        start, numel, shape, _ = self.parts[name]
        if name in self.odd:
            return after[start:start + numel].view(torch.int16)[:self.odd[name]].view(shape)
        if name in self.bf16:                      # bf16 bits
            return after[start:start + numel].view(torch.int16).view(shape)
        return after[start:start + numel].view(torch.float32).view(shape)

    def result(self, name):
        """The output `name` on the host, after checking that nothing outside the outputs changed."""
        return self.part(self.download(), name)

    def restore(self, **outputs):
        """The arena as uploaded, for another call on the same inputs; outputs named here start from the given contents
        (a float tensor, an int32 bit pattern - int16 for a bf16 part -, or None for the sentinel)."""
        for name, data in outputs.items():
            start, numel, _, out = self.parts[name]
            assert out
            if data is None:
                self.host[start:start + numel] = SENTINEL
            elif name in self.bf16:
                self.host[start:start + numel] = _bf16_words(data)
            else:
                flat = data.reshape(-1)
                self.host[start:start + numel] = flat if flat.dtype == torch.int32 else flat.float().view(torch.int32)
        self.dev.copy_(self.host)
        return self
