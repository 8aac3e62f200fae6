"""Writes tests/golden/stream.npz: what the LIVE six layers' ``online_inference`` returned for the chunk sequences of
``_stream_ref.GOLDEN_CASES`` (authoring container only: needs the real lhotse).

    python tests/_stream_golden.py

Per case ``<name>/x`` is the whole input and, per call i, ``<name>/<i>/out`` the output (``Wav2Win``: the frames, with ``<name>/<i>/log_energy``
when asked for), ``<name>/<i>/remainder`` the remainder that call returned.
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import _stream_ref as SR  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "stream.npz")


def main() -> None:
    from _dropin_support import import_lhotse

    import_lhotse()
    import lhotse.features.kaldi.layers as L

    arrays = {}
    for name in sorted(SR.GOLDEN_CASES):
        cls, kw, _, sizes = SR.GOLDEN_CASES[name]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            layer = getattr(L, cls)(**kw)
        x = SR.golden_input(name)
        arrays[f"{name}/x"] = x
        context = None
        for i, chunk in enumerate(SR.chunked(x, sizes)):
            with torch.no_grad():
                out, context = layer.online_inference(torch.from_numpy(chunk), context)
            if cls == "Wav2Win":
                out, log_e = out
                if log_e is not None:
                    arrays[f"{name}/{i}/log_energy"] = log_e.numpy()
            arrays[f"{name}/{i}/out"] = out.numpy()
            arrays[f"{name}/{i}/remainder"] = context.numpy()
    np.savez_compressed(GOLDEN, **arrays)
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes,", len(arrays), "arrays")


if __name__ == "__main__":
    main()
