"""What the tests of the shaped weight decay share (test_weight_decay_gpu.py, test_weight_decay_cli_cpu.py): decay masks packed on the host
independently of params.decay_mask_words, a step through mmego_adam_step_decay on the buffers of adam_helpers.AdamSet, and the error
of an fp32 tensor against float64 in units of ulp_fp32."""
import numpy as np
import torch

from adam_helpers import ADAM, LR, AdamSet


def pack_bits(bits):
    """One bool per float4 -> uint64 words, word w bit b = float4 64 w + b (plain Python integers: no packbits, no view)."""
    bits = [bool(b) for b in bits]
    words = []
    for w in range((len(bits) + 63) // 64):
        words.append(sum(1 << b for b, on in enumerate(bits[64 * w:64 * w + 64]) if on))
    return np.array(words, dtype=np.uint64)


def masks(n4, seed=11):
    """name -> bool array over the float4: all set, all clear, seeded runs of 1..70 float4 alternating set and clear (word and wave
    boundaries fall inside runs), only the last float4 set."""
    rng = np.random.default_rng(seed + n4)
    runs, on, total = [], True, 0
    while total < n4:
        k = int(rng.integers(1, 71))
        runs.append(np.full(k, on))
        on, total = not on, total + k
    last = np.zeros(n4, dtype=bool)
    last[-1] = True
    return {"set": np.ones(n4, dtype=bool), "clear": np.zeros(n4, dtype=bool), "runs": np.concatenate(runs)[:n4], "last": last}


_mask_cache = {}


def device_mask(dev, n, name):
    """(the words on the device as int64, the mask per ELEMENT as a bool tensor on the device); built once per (n, name).  The big
    run mask is packed with numpy to keep the test quick; tests/test_weight_decay_cli_cpu.py checks that packer against pack_bits."""
    key = (n, name)
    if key not in _mask_cache:
        bits = masks(n // 4)[name]
        if len(bits) <= 4096:
            words = pack_bits(bits)
        else:
            padded = np.zeros((len(bits) + 63) // 64 * 64, dtype=np.uint8)
            padded[:len(bits)] = bits
            words = np.packbits(padded, bitorder="little").view("<u8")
        _mask_cache[key] = (torch.from_numpy(words.view(np.int64).copy()).to(dev),
                            torch.from_numpy(np.repeat(bits, 4)).to(dev))
    return _mask_cache[key]


class DecaySet(AdamSet):
    def decay_step(self, g, wd, mask=None, decoupled=False, sched=None, decay=None, max_norm=None, skip=None, lr=LR):
        """One step through mmego_adam_step_decay in the form that (sched, decay, max_norm) select."""
        from mmego_amd import hip
        ns = 0 if skip is None else skip.numel() // 2
        clip = (None, 0, 0.0, None)
        if max_norm is not None:
            hip.call("grad_sqnorm", g, self.n, skip, ns, self.part, self.part.numel())
            clip = (self.part, self.part.numel(), max_norm, self.stats)
        avg = (None, 0.0) if decay is None else (self.ema, decay)
        hip.call("adam_step_decay", self.p, g, self.m, self.v, self.n, self.state, lr, *ADAM[1:], wd, skip, ns, self.ticket, *clip, *avg,
                 sched, mask, int(decoupled))


def ulp32(x64):
    """ulp_fp32 at |x| for a float64 tensor (normal range; below it the smallest normal's)."""
    _, e = torch.frexp(x64.abs().clamp_min(2.0 ** -126))          # |x| = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(x64), e - 24)


def worst_ulp(p32, p64):
    """max |p32 - p64| / ulp_fp32(|p64|), both on the host."""
    p64 = p64.double().cpu()
    return float(((p32.double().cpu() - p64).abs() / ulp32(p64)).max())
