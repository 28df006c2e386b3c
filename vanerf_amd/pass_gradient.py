"""Backward driver of a training step: `PassGradient` hands the HIP pass's images to autograd and, in backward, takes the gradient of
`vanerf_amd.torch_graph`'s networks at the samples of that pass, in two stages per chunk of rays.

(1) The composite stage turns the gradients of the images into the gradient with respect to every sample's [alpha, sdf, r, g, b]
    (and to sigmoid_beta): `vanerf_composite_backward` on the device, or a small torch graph over `torch_graph.composite`.
(2) A sample backend evaluates and differentiates the per-sample networks block of samples by block: the fused HIP backward
    (hip_backward.py, the default), replays of one captured graph (`_BlockGraph`), or the eager torch graph (`torch_graph.networks_at`, the
    independent checker of the first).
Samples are independent, so the gradient is the sum over blocks and only one block's activations exist at a time.  The per-frame vertex
table of TexVisFusion (two conv stacks over the source image) is shared by all samples: its graph is built once, the blocks accumulate the
gradient with respect to the table, and one backward through the stacks closes the step."""
from collections import namedtuple
from functools import partial

import torch

from . import hip_backward as HB
from . import renderer as R
from . import torch_graph as G

# Rays per chunk of the backward pass (PassGradient); None = the whole patch at once.  Chunking by rays repeats both stages per chunk; the block
# size below bounds memory more cheaply (it only cuts the second stage).  Measured on the 64x64 patch at 64 + 64 samples (
# tools/perf_train_step.py, one MI355X; 524 k network evaluations per step): whole patch 42 ms / 7.5 GiB; blocks of 262 144 samples 53 ms / 4.2 GiB;
# 131 072: 63 ms / 2.5 GiB.  With 288 GB of HBM the default is speed; model config keys `grad_rays_per_chunk`, `grad_samples_per_block`.
# (bf16 operands for this graph's GEMMs were measured too: 9 % faster, and the parameter gradients moved by 4e-2 relative -- dropped.)
GRAD_RAYS_PER_CHUNK = None
# Samples per block of the second stage of the backward pass (PassGradient); None = all samples of a chunk of rays in one block.
GRAD_SAMPLES_PER_BLOCK = None


def straight_through(value, graph):
    """HIP value, the torch graph's gradient."""
    return graph + (value - graph).detach()


class _Samples(namedtuple("_Samples", "pts q_sdf q_vis knn noise d noise2 d2")):
    """Every sample of a chunk of rays in one list, [coarse | new]: inputs of the networks, noise draws and the gradient `d` (n, 5) with respect
    to their outputs.  noise2 / d2: the second (noise, gradient) column, when the coarse points appear in the fine composite with other draws
    (zeros for the new samples there); None otherwise, as `noise` is without training noise."""
    __slots__ = ()

    def blocks(self, size):
        """(slice, that slice of every column) for blocks of `size` samples, the last one shorter."""
        n = self.pts.shape[0]
        for b0 in range(0, n, size):
            sl = slice(b0, min(n, b0 + size))
            yield sl, _Samples(*(None if t is None else t[sl] for t in self))


class _BlockGraph:
    """Second stage of PassGradient for blocks of ONE fixed size, captured once as a HIP graph and replayed block after block (config key
    `grad_graph_blocks`, with `grad_samples_per_block`).  Small blocks bound the step's memory, but eagerly every block re-launches the
    graph's ~2 000 kernels and the step turns host-bound (131 072 samples per block: 63 ms); replayed, a block costs the host a few input
    copies.  What capture needs: inputs, per-frame tensors and gradient accumulators at fixed addresses (copied in, read out), parameters that
    stay where they are (in-place optimizer updates; a moved parameter re-captures), no data-dependent shapes (the valid-sample compaction of
    networks_at is off inside: every sample of a block is evaluated)."""
    cache = {}

    def __init__(self, leaves, names, frame, table, block, two, with_noise, sp_args):
        dev = table.device
        zeros = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=dev)
        self.block = block
        # one block's samples, in _Samples' order
        self.inputs = _Samples(zeros(block, 3), zeros(block), zeros(block, dtype=torch.uint8), zeros(block, dtype=torch.int32),
                               zeros(block) if with_noise else None, zeros(block, 5), zeros(block) if two else None, zeros(block, 5) if two else None)
        # leaves: parameters are read where they live; the encoders' feature maps (new tensors every step) and the vertex table get fixed homes
        self.static = {n: (t.detach().clone() if n.startswith("@") else t.detach()).requires_grad_(True) for n, t in zip(names, leaves)}
        self.table = table.detach().clone().requires_grad_(True)
        self.frame = {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in frame.items() if k not in ("cam", "feat_geo", "feat_tex", "table29")}
        self.frame["cam"] = {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in frame["cam"].items()}
        order = list(self.static.values()) + [self.table]
        flat = zeros(sum(t.numel() for t in order))
        self.flat, self.acc, at = flat, [], 0
        for t in order:
            self.acc.append(flat[at:at + t.numel()].view(t.shape))
            at += t.numel()
        P = {k: v for k, v in self.static.items() if not k.startswith("@")}
        fr = dict(self.frame, feat_geo=[self.static["@feat_geo0"], self.static["@feat_geo1"]], feat_tex=self.static["@feat_tex"], table29=self.table)

        def body():
            s = self.inputs
            outs = G.networks_at(P, fr, s.pts, s.q_sdf, s.q_vis, s.knn.long(), (s.noise, s.noise2) if two else s.noise, sp_args, compact_valid=False)
            grads = torch.autograd.grad(list(outs) if two else outs, order, [s.d, s.d2] if two else s.d, allow_unused=True)
            for a, g in zip(self.acc, grads):
                if g is not None:
                    a.add_(g)

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.enable_grad():
            for _ in range(2):  # warm-up outside capture (library handles, workspaces, autotuning)
                body()
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.enable_grad(), torch.cuda.graph(self.graph):
            body()

    def begin(self, leaves, names, frame, table):
        """New step: this step's feature maps, per-frame tensors and vertex table into their fixed homes, accumulators to zero."""
        with torch.no_grad():
            for n, t in zip(names, leaves):
                if n.startswith("@"):
                    self.static[n].copy_(t)
            self.table.copy_(table)
            for k, v in self.frame.items():
                if torch.is_tensor(v):
                    v.copy_(frame[k])
            for k, v in self.frame["cam"].items():
                if torch.is_tensor(v):
                    v.copy_(frame["cam"][k])
            self.flat.zero_()

    def run(self, samples):
        n = samples.pts.shape[0]
        with torch.no_grad():
            for dst, src in zip(self.inputs, samples):
                if dst is not None:
                    dst[:n].copy_(src)
            if n < self.block:  # the last, shorter block: the tail keeps old samples with zero output gradients -- they add nothing
                self.inputs.d[n:].zero_()
                if self.inputs.d2 is not None:
                    self.inputs.d2[n:].zero_()
        self.graph.replay()

    def results(self):
        out = self.flat.clone()
        res, at = [], 0
        for a in self.acc:
            res.append(out[at:at + a.numel()].view(a.shape))
            at += a.numel()
        return res

    @classmethod
    def get(cls, leaves, names, frame, table, block, two, with_noise, sp_args):
        cam = frame["cam"]
        key = (block, two, with_noise, tuple(sorted(sp_args.items())), tuple(t.data_ptr() for n, t in zip(names, leaves) if not n.startswith("@")),
               tuple(tuple(t.shape) for n, t in zip(names, leaves) if n.startswith("@")), tuple((k, float(v)) for k, v in sorted(cam.items()) if not torch.is_tensor(v)),
               tuple((k, tuple(v.shape)) for k, v in sorted(frame.items()) if torch.is_tensor(v)), str(table.device))
        if key not in cls.cache:
            cls.cache.clear()  # one configuration at a time (each holds a block's activations in its private pool)
            cls.cache[key] = cls(leaves, names, frame, table, block, two, with_noise, sp_args)
        return cls.cache[key]


class _Step:
    """What one backward pass shares between its stages: the leaves (the module's parameters and the encoders' feature maps, detached copies
    that require grad) and their gradient accumulators `total`, the frame, the per-frame vertex table with its graph, and the accumulator
    `g_table` of the gradient with respect to the table."""

    def __init__(self, spec, saved):
        self.spec, self.names, self.saved, self.o = spec, spec["names"], list(saved), spec["pass"]
        self.leaves = [t.detach().requires_grad_(True) for t in saved]
        L = dict(zip(self.names, self.leaves))
        self.P = {k: v for k, v in L.items() if not k.startswith("@")}
        self.frame = dict(spec["frame"], feat_geo=[L["@feat_geo0"], L["@feat_geo1"]], feat_tex=L["@feat_tex"])
        self.total = [None] * len(self.leaves)
        self.table_graph = G.texture_vertex_table(self.P, G.project_vertices(self.frame["verts"], self.frame["cam"]), self.frame["feat_tex"], self.frame["img"])
        self.table = self.table_graph.detach().requires_grad_(True)
        self.g_table = torch.zeros_like(self.table)

    def accumulate(self, grads):
        """grads: one gradient or None per leaf, in the leaves' order."""
        for i, g in enumerate(grads):
            if g is not None:
                self.total[i] = g if self.total[i] is None else self.total[i] + g

    def ray_chunks(self):
        rays = self.o["z"].shape[0]
        size = self.spec["rays_per_chunk"] or rays
        return [(r0, min(rays, r0 + size)) for r0 in range(0, rays, size)]

    def close_table(self):
        """The one backward through the per-frame stacks."""
        self.accumulate(torch.autograd.grad(self.table_graph, self.leaves, self.g_table, allow_unused=True))


def _composite_gradients(step, gouts, r0, r1):
    """Stage 1 for rays r0:r1: the composites, differentiated at the HIP pass's own per-sample values -> (d_coarse, d_fine or None,
    d_coarse_in_fine or None), the gradients with respect to the [alpha, sdf, r, g, b] of the coarse samples, of the new samples of the fine
    batch, and of the coarse samples under the other draws they carry inside the fine batch.  sigmoid_beta's gradient goes into `step`."""
    o = step.o
    c, f = o["coarse"], o.get("fine")
    n_fine = 0 if f is None else (o["z_fine"].shape[1] if o.get("z_fine") is not None else f["rgba"].shape[1])
    # images are (1,3,h,w) / (1,h,w) over the patch's rays in row-major order: the chunk's rays are a slice of the flattened image
    gk = {k: (g.reshape(3, -1).t()[r0:r1] if k.startswith("tex_fg") else g.reshape(-1)[r0:r1]) for k, g in zip(step.spec["keys"], gouts) if g is not None}
    # On the device when the fused backward is configured, unless a composite has more than 256 samples per ray: vanerf_composite_backward keeps
    # a ray in one wave, four samples per lane at the most.  The forward has a one-thread-per-ray kernel for longer rays; the backward has torch.
    if step.spec.get("hip_backward") is not None and max(c["rgba"].shape[1], n_fine) <= 256:
        return _composite_gradients_hip(step, gk, slice(r0, r1))
    return _composite_gradients_torch(step, gk, slice(r0, r1))


@torch.no_grad()
def _composite_gradients_hip(step, gk, rays):
    """vanerf_composite_backward: one launch per composite instead of the torch graph's ~500 (rays x samples x 5 element-wise kernels, a cumprod
    whose backward blocks the host); sigmoid_beta is the handle's device copy (this step's parameter, clamped)."""
    o, w0 = step.o, step.spec["hip_backward"]["w0"]
    c, f = o["coarse"], o.get("fine")
    gk = {k: g.contiguous() for k, g in gk.items()}
    d_c, _, db = R.composite_backward(w0, c["rgba"][rays], o["z"][rays], c["q_sdf"][rays], gk.get("tex_fg"), gk.get("depth"), gk.get("alpha"))
    d_f = d_cf = None
    db = db.sum()
    if f is not None:
        gf = (gk.get("tex_fg_fine"), gk.get("depth_fine"), gk.get("alpha_fine"), gk.get("sdf"))
        if o.get("fine_src") is not None:  # merged [coarse | new]: the coarse entries are the coarse batch's own or, under noise, their other draws
            cf = o.get("coarse_in_fine")
            d_cf, d_f, db_f = R.composite_backward(w0, (c if cf is None else cf)["rgba"][rays], o["z_fine"][rays], c["q_sdf"][rays], *gf,
                                                   rgba_n=f["rgba"][rays], sdf_n=f["q_sdf"][rays], src=o["fine_src"][rays])
            if cf is None:
                d_c, d_cf = d_c + d_cf, None
        else:
            d_f, _, db_f = R.composite_backward(w0, f["rgba"][rays], o["z_fine"][rays], f["q_sdf"][rays], *gf)
        db = db + db_f.sum()
    pb = step.P["sigmoid_beta"]
    g_beta = [None] * len(step.leaves)
    g_beta[step.names.index("sigmoid_beta")] = (db * (pb.detach() >= 2e-3).to(db.dtype)).reshape(pb.shape)  # clamp(min = 2e-3)'s derivative
    step.accumulate(g_beta)
    return d_c, d_f, d_cf


def _composite_gradients_torch(step, gk, rays):
    """A small graph over (rays, samples, 5) tensors through torch_graph.composite."""
    o, P = step.o, step.P
    c, f = o["coarse"], o.get("fine")
    rc = c["rgba"][rays].detach().clone().requires_grad_(True)
    rf = rcf = None
    col, dep, acc, _ = G.composite(P, rc, o["z"][rays], c["q_sdf"][rays])
    outs = {"tex_fg": col, "depth": dep, "alpha": acc}
    if f is not None:
        rf = f["rgba"][rays].detach().clone().requires_grad_(True)
        rgba_f, msdf = rf, f["q_sdf"][rays]
        if o.get("fine_src") is not None:  # the pass re-used the coarse evaluations: merge [coarse | new] by the origin map
            src = o["fine_src"][rays].long()
            take = torch.where(src >= 0, src, rc.shape[1] + (-src - 1))
            merged = rc
            if o.get("coarse_in_fine") is not None:  # (training noise: the coarse points carry other draws inside the fine batch)
                merged = rcf = o["coarse_in_fine"]["rgba"][rays].detach().clone().requires_grad_(True)
            rgba_f = torch.gather(torch.cat([merged, rf], 1), 1, take[..., None].expand(-1, -1, 5))
            msdf = torch.gather(torch.cat([c["q_sdf"][rays], f["q_sdf"][rays]], 1), 1, take)
        col, dep, acc, sdf = G.composite(P, rgba_f, o["z_fine"][rays], msdf)
        outs.update({"tex_fg_fine": col, "depth_fine": dep, "alpha_fine": acc, "sdf": sdf})
    per_sample = [t for t in (rc, rf, rcf) if t is not None]
    grads = torch.autograd.grad([outs[k] for k in gk], per_sample + step.leaves, list(gk.values()), allow_unused=True)
    step.accumulate(grads[len(per_sample):])
    return tuple(grads[:len(per_sample)]) + (None,) * (3 - len(per_sample))


def _chunk_samples(o, d, r0, r1):
    """The samples of rays r0:r1 with stage 1's gradients `d` = (d_coarse, d_fine, d_coarse_in_fine) as one _Samples, [coarse | new]."""
    c, f = o["coarse"], o.get("fine")
    cf = o.get("coarse_in_fine") if f is not None else None
    rays, dev = o["z"].shape[0], c["pts"].device
    parts = []
    for part, d_part, noise2, d2 in ((c, d[0], None if cf is None else cf["noise"], d[2]), (f, d[1], None, None)):
        if part is None:
            continue
        S = part["pts"].shape[0] // rays
        sl = slice(r0 * S, r1 * S)
        zeros = lambda *width: torch.zeros(sl.stop - sl.start, *width, device=dev)
        noise = None if part["noise"] is None else part["noise"][sl]
        d_part = zeros(5) if d_part is None else d_part.reshape(-1, 5)
        if cf is None:
            noise2 = d2 = None
        else:  # the second column: the coarse samples' other draws; zeros for the new samples and for a gradient that autograd left unused
            noise2 = zeros() if noise2 is None else noise2[sl]
            d2 = zeros(5) if d2 is None else d2.reshape(-1, 5)
        parts.append(_Samples(part["pts"][sl], part["q_sdf"].reshape(-1)[sl], part["q_vis"][sl], part["knn"][sl], noise, d_part, noise2, d2))
    if len(parts) == 1:
        return parts[0]
    return _Samples(*(None if a is None else torch.cat([a, b], 0) for a, b in zip(*parts)))


class _FusedBackend:
    """Stage 2 on the fused HIP backward (csrc/query_backward.hip, hip_backward.py): two launches and twenty matrix products per block of
    samples; the input gradients of all blocks are scattered into the feature maps and the per-vertex tables, and finish() maps them and the
    flat weight-gradient accumulator to the leaves."""

    def __init__(self, step):
        self.step, self.hb, self.ws = step, step.spec["hip_backward"], None

    def add(self, s):
        step, hb, dev = self.step, self.hb, s.pts.device
        if self.ws is None:  # the first chunk of rays is a full one: its sample count bounds every later block
            self.block = min(int(hb["block"]), (s.pts.shape[0] + 31) // 32 * 32)
            self.ws = HB.workspace(self.block, dev)
            self.ws.dw.zero_()
            self.scatter = HB.InputScatter(step.frame, dev)
        with torch.no_grad():
            s = s._replace(pts=s.pts.contiguous(), q_sdf=s.q_sdf.contiguous(), q_vis=s.q_vis.contiguous(), knn=s.knn.contiguous())
            self.scatter.prepare(G.project(s.pts, step.frame["cam"])[0], s.knn)
            for sl, b in s.blocks(self.block):
                ig, _ = HB.run_block(self.ws, hb["w0"], hb["fdat"], b.pts, b.q_sdf, b.q_vis, b.knn, b.d, b.noise, b.d2, b.noise2)
                self.scatter.add(sl, ig)

    def finish(self):
        step, sc = self.step, self.scatter
        by_name = dict(HB.parameter_gradients(self.ws, step.P))
        by_name["@feat_geo0"], by_name["@feat_geo1"], by_name["@feat_tex"] = sc.map_gradient("map0"), sc.map_gradient("map1"), sc.map_gradient("tex")
        step.accumulate([by_name.get(n) for n in step.names])
        # the per-vertex tables are bilinear samples of the maps at the projected vertices (src/networks.py:86-87, 94-95): their gradient goes
        # back through that gather (and table29's through the per-frame stacks, in close_table)
        vert_xy = G.project_vertices(step.frame["verts"], step.frame["cam"])
        tabs = [G.sample_map(step.frame["feat_geo"][0], vert_xy), G.sample_map(step.frame["feat_geo"][1], vert_xy)]
        step.accumulate(torch.autograd.grad(tabs, step.leaves, [sc.acc["vtab0"], sc.acc["vtab1"]], allow_unused=True))
        step.g_table = step.g_table + sc.acc["table29"]


def _graph_add(step, s):
    """Stage 2 of one chunk as replays of one captured graph per block (_BlockGraph)."""
    args = (step.saved, step.names, step.frame, step.table)
    runner = _BlockGraph.get(*args, step.spec["samples_per_block"], s.noise2 is not None, s.noise is not None, step.spec["sp_args"])
    runner.begin(*args)
    for _, b in s.blocks(runner.block):
        runner.run(b)
    res = runner.results()
    step.accumulate(res[:-1])
    step.g_table += res[-1]


def _eager_add(step, s):
    """Stage 2 of one chunk on the eager torch graph: networks_at + torch.autograd.grad per block; only one block's graph exists at a time, which
    is what bounds the step's memory -- the coarse and the fine batch are never alive together."""
    two = s.noise2 is not None
    for _, b in s.blocks(step.spec.get("samples_per_block") or s.pts.shape[0]):
        outs = G.networks_at(step.P, dict(step.frame, table29=step.table), b.pts, b.q_sdf, b.q_vis, b.knn.long(), (b.noise, b.noise2) if two else b.noise,
                             step.spec["sp_args"])
        grads = torch.autograd.grad(list(outs) if two else outs, step.leaves + [step.table], [b.d, b.d2] if two else b.d, allow_unused=True)
        del outs
        step.accumulate(grads[:-1])
        if grads[-1] is not None:
            step.g_table += grads[-1]


def _sample_backend(step):
    """Stage 2 of this step -> (add(samples), finish()).  The two torch backends add into `step` block by block and have nothing to close."""
    spec = step.spec
    if spec.get("hip_backward") is not None:
        fused = _FusedBackend(step)
        return fused.add, fused.finish
    add = _graph_add if spec.get("graph_blocks") and spec.get("samples_per_block") else _eager_add
    return partial(add, step), lambda: None


class PassGradient(torch.autograd.Function):
    """forward: the HIP pass's images, unchanged.  backward: the gradients of torch_graph's networks at the samples of that pass with respect to
    the leaves (the module's parameters and the encoders' feature maps); the stages are described in the module header."""

    @staticmethod
    def forward(ctx, spec, *leaves):
        ctx.spec = spec
        ctx.save_for_backward(*leaves)
        return tuple(v.clone() for v in spec["values"])

    @staticmethod
    def backward(ctx, *gouts):
        with torch.enable_grad():
            step = _Step(ctx.spec, ctx.saved_tensors)
            add, finish = _sample_backend(step)
            for r0, r1 in step.ray_chunks():
                d = _composite_gradients(step, gouts, r0, r1)
                add(_chunk_samples(step.o, d, r0, r1))
            finish()
            step.close_table()
        return (None, *step.total)
