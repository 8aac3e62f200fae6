"""CPU: the routing rule of a rate pair (``lhotse_amd.augmentation.resample_route``) and the creation of a bankless resampler, without a
device.

* the dense-bank rule serves 1980 of the 9000 rate pairs 16000 <-> 2c, c = 3500 ... 7999 (LowpassUsingResampling's default cutoffs at
  16 kHz); the bankless kernel takes all the others;
* ``_sinc_bank_floats`` is the size of the bank ``constants.sinc_resample_kernel`` builds; the window cap is the header's;
* ``get_or_create_resampler`` of an over-threshold pair asks for the device's ``HipSincResampler`` while it holds the resampler cache's
  lock: the two caches must not share a lock (a device-free stand-in for the object; the call runs in a thread that is given up on
  instead of hanging the suite)."""
import threading

import torch

from lhotse_amd import augmentation as A
from lhotse_amd import constants as C


def test_the_dense_rule_serves_a_fifth_of_the_default_cutoffs_and_the_bankless_kernel_the_rest():
    pairs = [(16000, 2 * c) for c in range(3500, 8000)] + [(2 * c, 16000) for c in range(3500, 8000)]
    routes = [A.resample_route(*p) for p in pairs]
    assert sum(A._sinc_bank_floats(*p) <= A.MAX_RESAMPLE_BANK_FLOATS for p in pairs) == 1980
    assert routes.count("bank") == 1980 and routes.count("sinc") == 9000 - 1980 and None not in routes  # (the dense kernels take all 1980)
    # the dense kernel's own support rule is part of the route: a small bank whose hop does not fit its LDS is no "bank"
    assert A._sinc_bank_floats(16000, 202) <= A.MAX_RESAMPLE_BANK_FLOATS and not A._dense_kernel_fits(8000, 101, 476) and A.resample_route(16000, 202) is None
    assert A._dense_kernel_fits(441, 160, 17) and A._dense_kernel_fits(9, 10, 7) and A._dense_kernel_fits(1113, 1600, 7)
    # speed factors: 0.9 / 1.1 keep their banks, 1.037 at 16 kHz (1037 : 1000, 1 051 000 floats) has none
    assert A.resample_route(14400, 16000) == A.resample_route(17600, 16000) == "bank" and A.resample_route(16592, 16000) == "sinc"
    assert A.resample_route(16000, 9346) == A.resample_route(9346, 16000) == "sinc" and A._sinc_bank_floats(16000, 9346) == 4673 * 8022
    assert A.resample_route(48000, 7000) == "bank" and A.resample_route(48000, 7001) == "sinc"  # width 42, W = 86: under the cap
    assert A.resample_route(48001, 6000) is None  # W = 100
    assert A.resample_route(16000, 16000) is None and A.resample_route(0, 16000) is None and A.resample_route(16000, -1) is None
    for src, dst in ((44100, 16000), (17600, 16000), (16000, 22050), (8000, 16000)):
        kernel, width, orig, new = C.sinc_resample_kernel(src, dst)
        assert A._sinc_bank_floats(src, dst) == kernel.size and A._sinc_geometry(src, dst) == (orig, new, width) and A.resample_route(src, dst) == "bank"
    assert A.MAX_RESAMPLE_BANK_FLOATS == 1 << 20


def test_a_bankless_resampler_is_created_under_the_cache_lock_without_a_deadlock(monkeypatch):
    class Stand:  # (no device here)
        def __init__(self, device):
            self.device = device

    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(A, "HipSincResampler", Stand)
    monkeypatch.setattr(A, "_sincs", {})
    monkeypatch.setattr(A, "_precompiled_resamplers", {})
    got = {}

    def work():
        r = A.get_or_create_resampler(11127, 16000, "cuda:0")
        got.update(name=r.kernel_name, kernel=r.kernel, dims=(r.orig, r.new, r.width), sinc=r.sinc, again=A.get_or_create_resampler(11127, 16000, "cuda:0") is r)

    t = threading.Thread(target=work, daemon=True)
    t.start()
    t.join(30)
    assert not t.is_alive(), "get_or_create_resampler did not return: the caches share a lock"
    assert got["name"] == "resample_sinc" and got["kernel"] is None and got["dims"] == (11127, 16000, 7) and got["again"]
    assert isinstance(got["sinc"], Stand) and A.get_or_create_sinc("cuda:0") is got["sinc"]
