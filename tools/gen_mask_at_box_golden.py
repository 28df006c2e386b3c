"""Writes tests/golden/mask_at_box.npz by RUNNING THE REFERENCE'S OWN CODE on the CPU: Dataset.get_mask_at_box (src/dataset.py:122-129) for
synthetic target cameras and Dataset.load_human_bounds_pred (src/dataset.py:131-138) for one vertex set.  Build-machine only (it imports the
reference through oracle.ref_import); never runs where the GPU tests run and is never imported by the product path.

    python tools/gen_mask_at_box_golden.py

Per case `n` the file holds the inputs `n/K`, `n/R`, `n/T` ((V, 3, 3), (V, 3, 3), (V, 3)), `n/bounds` (2, 3), all fp32, `n/H`, `n/W`, and the
reference's outputs `n/mask` (V, H, W) uint8, `n/near_min`, `n/far_max` (V,) fp64.  The reference is called with the fp32 matrices widened
to fp64, so that it forms the rays in fp64 as the definition does, and with the fp32 bounds.  `bounds_pred/verts`, `bounds_pred/bounds`: the bounds
case.

Before anything is written the fp64 restatement of tests/test_mask_at_box.py is held to the reference on every case: masks equal outside the
near-threshold pixels, which may be at most 0.5 % of a case, and near_min / far_max within 1e-6 relative."""
import importlib.util
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "tests", "golden", "mask_at_box.npz")


def _test_module():
    spec = importlib.util.spec_from_file_location("test_mask_at_box", os.path.join(REPO, "tests", "test_mask_at_box.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cases(tm, bounds):
    """name -> (H, W, [(K, R, T), ...]).  Focal lengths are chosen so that the box covers between 20 % and 80 % of each image (asserted below)."""
    centre = bounds.astype(np.float64).mean(0)
    out = {}
    # identity rotation, the principal point on the centre of pixel (2, 3), the box centre on the axis: the central ray has d_x = d_y = 0
    T = (-centre + np.array([0.0, 0.0, 0.6])).astype(np.float32)
    out["7x5"] = (7, 5, [(tm.pinhole(9.0, 2.0, 3.0), np.eye(3, dtype=np.float32), T)])
    out["40x21"] = (40, 21, [(tm.pinhole(52.0, 9.7, 20.4),) + tm.look_at(centre + np.array([0.35, -0.25, 0.55]), centre + np.array([0.01, 0.0, -0.01]), roll=0.3)])
    inside = tm.look_at(centre + np.array([0.01, -0.005, 0.02]), centre + np.array([0.3, 0.2, 1.0]), roll=-0.2)
    out["3x70x45"] = (70, 45, [
        (tm.pinhole(95.0, 21.3, 36.1),) + tm.look_at(centre + np.array([-0.5, 0.3, 0.45]), centre, roll=-0.5),
        (tm.pinhole(60.0, 22.0, 35.0),) + inside,
        (tm.pinhole(130.0, 30.5, 28.0),) + tm.look_at(centre + np.array([0.1, 0.7, -0.5]), centre + np.array([0.0, 0.02, 0.0]), roll=1.1)])
    out["334x512"] = (334, 512, [(tm.pinhole(760.0, 250.4, 170.8),) + tm.look_at(centre + np.array([0.45, 0.2, -0.7]), centre, roll=0.15)])
    return out


def main():
    tm = _test_module()
    from oracle.ref_import import import_reference
    import_reference()  # (changes the working directory: every path above is absolute)
    from src.dataset import Dataset

    rng = np.random.RandomState(7)
    verts = (np.array([0.04, -0.02, 0.85]) + rng.uniform(-1.0, 1.0, (96, 3)) * np.array([0.11, 0.08, 0.05])).astype(np.float32)
    bounds = Dataset.load_human_bounds_pred(None, verts.copy())
    assert bounds.dtype == np.float32 and bounds.shape == (2, 3)
    arrs = {"bounds_pred/verts": verts, "bounds_pred/bounds": bounds}
    for name, (H, W, cams) in cases(tm, bounds).items():
        K, R, T = (np.stack([c[i] for c in cams]).astype(np.float32) for i in range(3))
        masks, nears, fars = [], [], []
        for v in range(len(cams)):
            mask, near, far = Dataset.get_mask_at_box(bounds.copy(), K[v].astype(np.float64), R[v].astype(np.float64), T[v].astype(np.float64), H, W)
            masks.append(mask.astype(np.uint8)), nears.append(float(near)), fars.append(float(far))
        for v, row in enumerate(tm.table_rows(K, R, T)):
            ref = tm.restate(row, bounds, H, W)
            what = f"{name}[{v}]"
            tm.masks_agree(ref.mask, masks[v], ref.unsure, what)
            rel = max(abs(ref.near_min - nears[v]) / nears[v], abs(ref.far_max - fars[v]) / fars[v])
            cover = masks[v].mean()
            print(f"{what}: cover {cover:.3f}  excluded {ref.unsure.mean():.5f}  differing {int((ref.mask != (masks[v] != 0)).sum())}  near/far rel {rel:.2e}")
            assert rel <= tm.TOL_REFERENCE, what
            assert 0.2 <= cover <= 0.8 or (name == "3x70x45" and v == 1 and cover == 1.0), (what, cover)
        arrs.update({f"{name}/K": K, f"{name}/R": R, f"{name}/T": T, f"{name}/bounds": bounds, f"{name}/H": np.int32(H), f"{name}/W": np.int32(W),
                     f"{name}/mask": np.stack(masks), f"{name}/near_min": np.array(nears), f"{name}/far_max": np.array(fars)})
    np.savez_compressed(OUT, **arrs)
    size = os.path.getsize(OUT)
    largest = max(os.path.getsize(os.path.join(os.path.dirname(OUT), f)) for f in os.listdir(os.path.dirname(OUT)) if f != os.path.basename(OUT))
    print(f"{OUT}: {size / 1024:.1f} KiB (the largest other fixture: {largest / 1024:.1f} KiB)")
    assert size < largest


if __name__ == "__main__":
    main()
