"""Writes tests/golden/weight_stream_digests.json: the SHA-256 of every host stream of the weight packer (`which` 0..6 of
vanerf_weights_stream_host) and of vanerf_weights_pack_host's stream, with its offsets list, for two state dicts -- the golden hot weights and
the same dict with every tensor's elements reversed in flattened order (a pure permutation: the same bits anywhere).
tests/test_weight_streams.py recomputes them.  Run it with the library of the commit whose bytes are to be pinned, BEFORE changing the packer."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "tests", "golden", "weight_stream_digests.json")
NUM_STREAMS = 7


def state_dicts():
    with np.load(os.path.join(REPO, "tests", "golden", "weights_hot.npz")) as z:
        sd = {k: torch.from_numpy(z[k]) for k in z.files}
    return {"hot": sd, "reversed": reversed_state_dict(sd)}


def reversed_state_dict(sd):
    return {k: t.flatten().flip(0).view_as(t).contiguous() for k, t in sd.items()}


def _sha(t):
    return hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()


def digests(sd):
    from vanerf_amd import renderer
    stream, offs = renderer.pack_weights_host(sd)
    return {"streams": [_sha(renderer.stream_host(sd, which)) for which in range(NUM_STREAMS)],
            "pack_host": _sha(stream), "pack_host_offsets": [int(o) for o in offs]}


if __name__ == "__main__":
    with open(OUT, "w") as f:
        json.dump({name: digests(sd) for name, sd in state_dicts().items()}, f, indent=1)
        f.write("\n")
    print(OUT)
