"""Writes tests/golden/mlp_forward_parent_bits.npz: seeded inputs, weights and the outputs of the split forward kernels for
N = 513 samples, K0 = 36 and 52 inputs, both piece forms (two fp16 pieces, three bf16 pieces), as the library in use computes
them.  Run it ONCE on the GPU with the library of the commit whose results are to be pinned.  PSDF_LIB_PATH must name that
library (the tool refuses the in-tree default, which is whatever was built last) and COMMIT the commit it was built from;
both are recorded in the file (`generated_from_commit`, and `library_sha256` of the shared library), so the claim "these are
the parent's bits" can be audited by rebuilding that commit:

    PSDF_LIB_PATH=/path/to/libpsdf_hip.so python tools/make_mlp_forward_golden.py OUT.npz COMMIT

tests/test_gpu_mlp_forward_forms.py asserts byte equality of every workgroup form against the file."""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from permuto_sdf_amd.mlp import mlp_forward_raw, pack_params  # noqa: E402

N = 513


def main(out, commit):
    lib = os.environ.get("PSDF_LIB_PATH")
    if not lib or not os.path.exists(lib):
        raise SystemExit("PSDF_LIB_PATH must name the library of the commit whose results are pinned")
    if len(commit) != 40 or any(c not in "0123456789abcdef" for c in commit):
        raise SystemExit("COMMIT must be the full 40-digit id of the commit the library was built from")
    dev = torch.device("cuda")
    doc = {"generated_from_commit": np.array(commit),
           "library_sha256": np.array(hashlib.sha256(open(lib, "rb").read()).hexdigest())}
    for K0 in (36, 52):
        g = torch.Generator().manual_seed(1000 + K0)
        dims = [K0, 64, 64, 64, 1]
        x = torch.randn(K0, N, generator=g)
        x[K0 // 2:] *= 1e-3                      # encoding-like: small channels beside large ones
        ws = [(torch.rand(dims[i + 1], dims[i], generator=g) * 2 - 1) * (6.0 / (dims[i] + dims[i + 1])) ** 0.5 for i in range(4)]
        bs = [(torch.rand(dims[i + 1], generator=g) * 2 - 1) * 0.1 for i in range(4)]
        doc["x_%d" % K0] = x.numpy()
        for i in range(4):
            doc["w%d_%d" % (i, K0)] = ws[i].numpy()
            doc["b%d_%d" % (i, K0)] = bs[i].numpy()
        xd, wd, bd = x.to(dev).contiguous(), [w.to(dev) for w in ws], [b.to(dev) for b in bs]
        for name, f16 in (("f16", True), ("bf16", False)):
            y = mlp_forward_raw(dims, xd, pack_params(dims, wd, bd, f16=f16), f16=f16)
            torch.cuda.synchronize()
            doc["y_%s_%d" % (name, K0)] = y.cpu().numpy()
    np.savez(out, **doc)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
