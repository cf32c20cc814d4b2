#!/usr/bin/env python
"""Freeze the LIVE reference's KG2E / HoLE outputs into tests/golden/ref_{kg2e,kg2e_clip,hole}.npz (build container only:
oracle/make_golden.py imports the reference tree through oracle/ref_shim.py).  The recipe is oracle/make_golden.py's
golden_for, called unchanged.  Fixed seeds: a second run writes identical arrays.

  kg2e       the reference's defaults cmax = 0.05, cmin = 5.0 (swapped): every sigma entry starts at exactly 5.0
  kg2e_clip  cmax = 5.0, cmin = 0.05: sigma starts at xavier + 1, so the rows and their norms vary
  hole       HoLE.forward calls the torch < 1.7 API (torch.fft(x, 1) / torch.ifft(x, 1) on real [..., 2] tensors).  For the
             duration of the call a compatibility shim makes torch.fft callable with those semantics (torch.fft.* stays
             reachable) and adds torch.ifft (1/n scaling); torch is restored afterwards.  The shim lives here only.

Usage:  python tools/make_golden_kg2e_hole.py [kg2e|kg2e_clip|hole ...]
"""
import contextlib
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import make_golden  # noqa: E402
import torch  # noqa: E402

CASES = {
    "kg2e": ("pairwise.KG2E", dict(hidden_size=16, cmax=0.05, cmin=5.0, margin=1.0), 3201, False),
    "kg2e_clip": ("pairwise.KG2E", dict(hidden_size=16, cmax=5.0, cmin=0.05, margin=1.0), 3202, False),
    "hole": ("pairwise.HoLE", dict(hidden_size=16, cmax=0.05, cmin=5.0, margin=1.0), 3203, True),
}


class _LegacyFFT(types.ModuleType):
    """torch.fft as a module that is also the torch < 1.7 function fft(input, signal_ndim) (signal_ndim = 1 only)."""

    def __init__(self, mod):
        super().__init__(mod.__name__)
        self.__dict__.update({k: v for k, v in mod.__dict__.items() if k != "__name__"})
        self._mod = mod

    def __call__(self, x, signal_ndim):
        assert signal_ndim == 1
        return torch.view_as_real(self._mod.fft(torch.view_as_complex(x.contiguous())))


@contextlib.contextmanager
def legacy_fft():
    mod = torch.fft
    had_ifft = hasattr(torch, "ifft")

    def ifft(x, signal_ndim):
        assert signal_ndim == 1
        return torch.view_as_real(mod.ifft(torch.view_as_complex(x.contiguous())))   # norm="backward": 1/n

    torch.fft = _LegacyFFT(mod)
    torch.ifft = ifft
    try:
        yield
    finally:
        torch.fft = mod
        if not had_ifft:
            del torch.ifft


if __name__ == "__main__":
    only = set(sys.argv[1:])
    for name, (cls_path, hp, seed, shim) in CASES.items():
        if only and name not in only:
            continue
        with legacy_fft() if shim else contextlib.nullcontext():
            make_golden.golden_for(name, cls_path, hp, seed)
