"""What the GPU tests of the fused Adam step share (test_clip_grad_norm_gpu.py, test_ema_gpu.py, test_lr_schedule_gpu.py): the buffers of one
optimiser with a step through every entry point of csrc/optim.hip, the comparison on bit patterns and the seeded gradients."""
import torch

LR = 3e-5
ADAM = (LR, 0.9, 0.999, 1e-8)
_INT_OF_SIZE = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def same_bits(a, b):
    """torch.equal on the bit patterns (NaN-safe, and -0.0 is not 0.0); where both are on the device, there."""
    if a.device != b.device:
        a, b = a.cpu(), b.cpu()
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(_INT_OF_SIZE[a.element_size()]),
                                              b.contiguous().view(_INT_OF_SIZE[b.element_size()]))


_grad_cache = {}


def grads(dev, n, steps, seed=5):
    """(p0, [g_1 .. g_steps]) on the device: seeded, a fresh gradient per step; computed once per (n, steps) and never written."""
    key = (n, steps, seed)
    if key not in _grad_cache:
        g = torch.Generator(device=dev).manual_seed(seed + n)
        _grad_cache[key] = (torch.randn(n, device=dev, generator=g), [torch.randn(n, device=dev, generator=g) * 0.1 for _ in range(steps)])
    return _grad_cache[key]


class AdamSet:
    """p, m, v, state (``words`` doubles: 3, or 4 for the scheduled step), ticket, the records and statistics of the clipped step and the
    average of one optimiser, on the device.  p0 may lie on the host."""

    def __init__(self, dev, p0, words=3):
        from mmego_amd import hip
        n = self.n = p0.numel()
        self.p, self.m, self.v = p0.clone().to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        self.ema = self.p.clone()
        self.state = torch.zeros(words, dtype=torch.float64, device=dev)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        self.part = torch.zeros(hip.lib().mmego_grad_norm_nblk(n), dtype=torch.float64, device=dev)
        self.stats = torch.zeros(8, dtype=torch.float64, device=dev)

    def step(self, g, wd, decay=None, max_norm=None, skip=None, lr=LR):
        """One step through the unscheduled entry point that (decay, max_norm) select, at the rate ``lr``."""
        from mmego_amd import hip
        ns = 0 if skip is None else skip.numel() // 2
        avg = () if decay is None else (self.ema, decay)
        sfx = "" if decay is None else "_ema"
        if max_norm is None:
            hip.call("adam_step" + sfx, self.p, g, self.m, self.v, self.n, self.state, lr, *ADAM[1:], wd, skip, ns, self.ticket, *avg)
        else:
            hip.call("grad_sqnorm", g, self.n, skip, ns, self.part, self.part.numel())
            hip.call("adam_step_clipped" + sfx, self.p, g, self.m, self.v, self.n, self.state, lr, *ADAM[1:], wd, skip, ns, self.ticket,
                     self.part, self.part.numel(), max_norm, self.stats, *avg)

    def sched_step(self, g, wd, sched, decay=None, max_norm=None, skip=None):
        """One step through mmego_adam_step_sched in the form that (decay, max_norm) select."""
        from mmego_amd import hip
        ns = 0 if skip is None else skip.numel() // 2
        clip = (None, 0, 0.0, None)
        if max_norm is not None:
            hip.call("grad_sqnorm", g, self.n, skip, ns, self.part, self.part.numel())
            clip = (self.part, self.part.numel(), max_norm, self.stats)
        avg = (None, 0.0) if decay is None else (self.ema, decay)
        hip.call("adam_step_sched", self.p, g, self.m, self.v, self.n, self.state, *ADAM, wd, skip, ns, self.ticket, *clip, *avg, sched)

    def tensors(self):
        return (self.p, self.m, self.v, self.ema, self.stats)

    def snapshot(self, stats=False, ema=False):
        """Copies of [p, m, v, state], then the statistics and the average where asked for."""
        torch.cuda.synchronize()
        return [t.clone() for t in (self.p, self.m, self.v, self.state) + ((self.stats,) if stats else ()) + ((self.ema,) if ema else ())]

    def same_adam(self, other):
        """p, m, v and the whole state equal as bit patterns; ``other``: another set, or a snapshot()."""
        return all(same_bits(a, b) for a, b in zip(self.snapshot(), other.snapshot() if isinstance(other, AdamSet) else other))

    def same(self, other):
        """p, m, v, ema, stats and state[0..2] equal as bit patterns (a scheduled set against an unscheduled one: three words against four)."""
        torch.cuda.synchronize()
        return all(same_bits(a, b) for a, b in zip(self.tensors(), other.tensors())) and same_bits(self.state[:3], other.state[:3])
