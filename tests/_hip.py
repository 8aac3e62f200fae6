"""Helpers for the GPU tests: build Hip* extractors from golden-case descriptions."""
from __future__ import annotations

import warnings

import numpy as np
import torch

import lhotse_amd as LA

_TABLE = {
    "fbank": (LA.HipFbank, LA.HipFbankConfig),
    "mfcc": (LA.HipMfcc, LA.HipMfccConfig),
    "spectrogram": (LA.HipSpectrogram, LA.HipSpectrogramConfig),
    "log-spectrogram": (LA.HipLogSpectrogram, LA.HipLogSpectrogramConfig),
}


_HOST_REGISTER = None


def host_register_supported() -> bool:
    """Can GPU 0's runtime page-lock memory the caller already has (hipHostRegister behind hipfeat_host_register)?  Asked once, with one
    anonymous page.  Some machines (virtual ones among them) cannot: there the ring's slots stay on the staging route, as after any other
    refused registration.  Only the RUNTIME's refusal counts as "unsupported": any other failure of the call is raised."""
    global _HOST_REGISTER
    if _HOST_REGISTER is None:
        import mmap

        from lhotse_amd import _lib

        lib = _lib.load()
        m = mmap.mmap(-1, mmap.PAGESIZE)
        page = np.frombuffer(m, dtype=np.uint8)
        try:
            lib.check("hipfeat_host_register", 0, page.ctypes.data, page.shape[0])
            lib.check("hipfeat_host_unregister", page.ctypes.data)
            _HOST_REGISTER = True
        except _lib.HipFeatError as e:
            if "hipHostRegister(" not in str(e):
                raise
            _HOST_REGISTER = False
        del page
        m.close()
    return _HOST_REGISTER


def make_hip(kind: str, cfg: dict, **extra):
    cls, ccls = _TABLE[kind]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return cls(ccls(**cfg, **extra))


def run_case(case, waves, want_kernel=False):
    """Run the HIP path through the same entry point the reference was run through."""
    outs, ex = _run_case(case, waves)
    return (outs, ex.kernel_name) if want_kernel else outs


def _run_case(case, waves):
    sr = case["cfg"].get("sampling_rate", 16000)
    if case["mode"] == "extract":
        ex = make_hip(case["kind"], case["cfg"])
        return [ex.extract(w, sr) for w in waves], ex
    ex = make_hip(case["kind"], case["cfg"], edge_rule="batch_zero_pad")
    if case["mode"] == "batch":
        res = ex.extract_batch(list(waves), sr)
        return (list(res) if not (isinstance(res, np.ndarray) and res.ndim == 2) else [res]), ex
    lens = torch.tensor([len(w) for w in waves], dtype=torch.int32)
    padded = torch.zeros(len(waves), int(lens.max()))
    for i, w in enumerate(waves):
        padded[i, : len(w)] = torch.from_numpy(w)
    return list(ex.extract_batch(padded, sr, lengths=lens)), ex
