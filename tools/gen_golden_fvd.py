"""Records what the FVD tests hold the restatement against, from the upstream reference (through tools/ref_shim.py; build container only):
  tests/golden/fvd_chunks.npz       calculate_n_chunks for 1 .. 128 frames: the chunk count, the drop flag, and where the reference raises
  tests/golden/fvd_blocks.npz       float64 outputs of Unit3D, MaxPool3dSamePadding and InceptionModule at thin widths; inputs and weights
                                    are regenerated from the seeds of tests/fvd_ref.py, so only the outputs are stored
  tests/golden/fvd_network.npz      float64 InceptionI3d.extract_features at the real widths on one seeded 9-frame clip (weights from seeds too)
  tests/golden/fvd_wasserstein.npz  calculate_2_wasserstein_dist on the seeded feature tables of tests/fvd_ref.py, next to the reference's
                                    own deviation from the float64 singular-value form (its non-symmetric eigvals is noisy)
Usage: python tools/gen_golden_fvd.py"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fvd_ref  # noqa: E402
import ref_shim  # noqa: E402
from vp_suite_amd import measure as M  # noqa: E402


def save(name, arrays):
    path = os.path.join(ROOT, "tests", "golden", f"{name}.npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size <= 200 * 1024, f"{name}.npz is larger than 200 KB"
    print(f"{name}.npz: {len(arrays)} arrays, {size} bytes")


def chunks(fvd):
    rows = []
    for T in range(1, fvd_ref.CHUNK_MAX_T + 1):
        try:
            n, drop = fvd.FrechetVideoDistance.calculate_n_chunks(types.SimpleNamespace(_MIN_T=9, _MAX_T=16), T)
            rows.append((T, n, int(drop), 0))
        except TypeError:
            rows.append((T, 0, 0, 1))
    return {"table": np.asarray(rows, dtype=np.int64)}


def load_unit(unit, tensors, name):
    unit.load_state_dict({k[len(name) + 1:]: v for k, v in tensors.items() if k.startswith(name + ".")})


def blocks(i3d):
    out = {}
    for case in fvd_ref.UNIT_CASES:
        ci, co, k, s, shape = case
        x, tensors = fvd_ref.unit_case(case)
        u = i3d.Unit3D(ci, co, kernel_shape=list(k), stride=s, name="u")
        load_unit(u, tensors, "u")
        out["unit_" + fvd_ref.case_id(case)] = u.double().eval()(x.double()).detach().numpy()
    for case in fvd_ref.POOL_CASES:
        k, s, shape, kind = case
        out["pool_" + fvd_ref.case_id(case)] = i3d.MaxPool3dSamePadding(kernel_size=list(k), stride=s, padding=0)(fvd_ref.pool_case(case).double()).numpy()
    for case in fvd_ref.BLOCK_CASES:
        ci, widths, shape = case
        x, tensors = fvd_ref.block_case(case)
        m = i3d.InceptionModule(ci, list(widths), "m")
        for b, _ in M.FVD_BRANCHES:
            load_unit(getattr(m, b), tensors, f"m.{b}")
        out["block_" + fvd_ref.case_id(case)] = m.double().eval()(x.double()).detach().numpy()
    return out


def network(i3d):
    net = i3d.InceptionI3d(num_classes=fvd_ref.N_FEATURES, in_channels=3)
    net.load_state_dict(fvd_ref.state_dict(1))
    feats = net.double().eval().extract_features(fvd_ref.network_case().double().permute(0, 2, 1, 3, 4))
    assert tuple(feats.shape) == (1, fvd_ref.N_FEATURES, 1, 1, 1)
    return {"features": feats.reshape(1, -1).numpy()}


def wasserstein(fvd):
    out = {}
    for b, n, kind in fvd_ref.WASSERSTEIN_CASES:
        p, t = fvd_ref.feature_tables(b, n, kind)
        ref = fvd.calculate_2_wasserstein_dist(p, t)
        assert ref.dtype == torch.float32
        dev = abs(float(ref) - float(M.frechet_distance_host(p, t)))
        print(f"b={b} n={n} {kind}: reference {float(ref):.9e}, deviation from the svdvals form {dev:.3e}")
        out[f"{b}_{n}_{kind}"] = np.asarray([float(ref), dev], dtype=np.float64)
    return out


def main():
    ref_shim.load_reference()
    import vp_suite.measure.fvd._pytorch_i3d.pytorch_i3d as i3d
    import vp_suite.measure.fvd.fvd as fvd
    with torch.no_grad():
        save("fvd_chunks", chunks(fvd))
        save("fvd_blocks", blocks(i3d))
        save("fvd_network", network(i3d))
        save("fvd_wasserstein", wasserstein(fvd))


if __name__ == "__main__":
    main()
