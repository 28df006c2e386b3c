"""Every byte of every stream a weight handle can carry (include/vanerf_hip.h, VANERF_STREAM_*).
On the CPU: the host packer's streams against SHA-256 digests recorded before the packer was reorganised around one table of streams
(tests/golden/weight_stream_digests.json, written by tools/gen_stream_digests.py).  On the GPU: what a handle holds after a pack and after an
update in place against the host packer, stream by stream, and the refusals of vanerf_weights_download."""
import importlib.util
import json
import os
from ctypes import byref, c_int64

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHICH = range(7)
CARRIED = {"fp32": {0: 0, 2: 2}, "bf16x3": {0: 1, 3: 3, 4: 4, 5: 5, 6: 6}}  # mode -> {which of the download: which of the host stream}


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("gen_stream_digests", os.path.join(REPO, "tools", "gen_stream_digests.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name", ["hot", "reversed"])
def test_host_streams_keep_their_bytes(gen, name):
    with open(os.path.join(REPO, "tests", "golden", "weight_stream_digests.json")) as f:
        want = json.load(f)[name]
    got = gen.digests(gen.state_dicts()[name])
    assert len(want["streams"]) == len(WHICH) and len(set(want["streams"])) == len(WHICH)  # seven streams, no two alike
    assert got == want


def test_stream_names_are_the_abi_numbers():
    from vanerf_amd import renderer as R
    hdr = open(os.path.join(REPO, "include", "vanerf_hip.h")).read()
    for name, which in R.STREAMS.items():
        assert f"VANERF_STREAM_{name.upper()} = {which}" in hdr, name
    assert sorted(R.STREAMS.values()) == list(WHICH)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_device_streams_equal_the_host_streams_after_pack_and_update(gen, precision):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from vanerf_amd import renderer as R
    from vanerf_amd._ffi import VanerfError, lib
    sds = gen.state_dicts()
    host = {name: [R.stream_host(sd, which) for which in WHICH] for name, sd in sds.items()}
    assert all(not torch.equal(a, b) for a, b in zip(host["hot"], host["reversed"]))  # the update below changes every stream
    w = R.PackedWeights(sds["hot"], mode=precision)
    carried = CARRIED[precision]
    n = c_int64()
    for name in ("hot", "reversed"):
        if name == "reversed":
            w.update({k: v.cuda() for k, v in sds[name].items()})
        for which in WHICH:
            if which in carried:
                assert torch.equal(R.stream_device(w, which), host[name][carried[which]]), (name, which)
            else:
                assert lib.vanerf_weights_download(w.handle, which, None, 0, byref(n)) == -22, (name, which)
                want = b"which = 1" if which == 1 else b"carries no such stream"
                assert want in lib.vanerf_last_error(), (name, which)
    for which in (-1, 7, 1 << 20):
        assert lib.vanerf_weights_download(w.handle, which, None, 0, byref(n)) == -22 and b"which = " in lib.vanerf_last_error()
        with pytest.raises(VanerfError, match="which = "):
            R.stream_host(sds["hot"], which)
    w.close()
