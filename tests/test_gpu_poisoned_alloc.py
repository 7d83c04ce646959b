"""No result may depend on what ``torch.empty`` returns (-m gpu).

The Python layer of sapcu_amd hands some ninety ``torch.empty`` / ``empty_like`` / ``new_empty`` buffers to the HIP library as
outputs, gradients, statistics, index tables, masks and workspaces.  Each is right only if the kernels behind it store every
element that is read later.  Every scenario here runs the same code three times from the same seeds and freshly built models and
optimisers — clean, then with every such buffer pre-filled with pattern A, then with pattern B (tests/poison.py) — and everything
the caller can see must be bit-identical (``torch.equal`` on the integer view of floating tensors, so NaNs and f64 compare by
their bits): outputs, kNN tables, taps, losses, gradients, parameters, buffers, optimiser state.  The clean run is the one the
rest of the suite ties to the oracle, so there is no tolerance here.

The last test holds the call sites the proxy recorded against ``SITES`` (tests/test_poison_host.py): every site was reached
under both patterns or stands in ``EXEMPT`` with its reason.  A new ``torch.empty`` in the package fails that test until a
scenario here reaches it: add the call that runs it to the scenario of its file and return what it computes."""
import numpy as np
import pytest
import torch

import gpu_utils as U
import poison
from conftest import FD_KW, FN_KW, golden
from test_poison_host import SITES

pytestmark = pytest.mark.gpu

F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64
PRECISIONS = ("f32", "bf16")
FD_OP_SHAPES = ((3, 7, 5, 96), (1, 33, 33, 64))           # (P, M, kk, C)

# site -> why no scenario of this file can reach it (at most one site in ten)
EXEMPT = {
    ("dist.py", 154): "needs two ranks: only a rank other than 0 receives the broadcast seeds into a new buffer",
}

_EXPECTED = {}                                             # test name -> its cases; _RAN: those that ran to the end
_RAN = {}
_CACHE = {}


def _expect(name, cases=(None,)):
    _EXPECTED[name] = set(cases)


def _done(name, case=None):
    _RAN.setdefault(name, set()).add(case)


def _dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return t.to(device=U.dev(), dtype=dtype) if dtype is not None else t.to(U.dev())


def _bits(t):
    """The integer view of a floating tensor (tests/test_cloud_sharded.py::_bits for every width), anything else as it is."""
    t = t.detach().contiguous()
    if t.dtype.is_floating_point:
        return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
    return t


def _flatten(value, prefix, out):
    if isinstance(value, dict):
        for k in value:
            _flatten(value[k], "%s/%s" % (prefix, k), out)
    elif isinstance(value, (list, tuple)):
        for i, v in enumerate(value):
            _flatten(v, "%s[%d]" % (prefix, i), out)
    elif isinstance(value, np.ndarray):
        out[prefix] = torch.from_numpy(np.ascontiguousarray(value))
    elif isinstance(value, float):
        out[prefix] = torch.tensor(value, dtype=F64)
    else:
        out[prefix] = value                                # a tensor, None, an int, a bool, a string
    return out


def _assert_same(clean, got, what):
    a, b = _flatten(clean, "", {}), _flatten(got, "", {})
    assert list(a) == list(b), (what, sorted(set(a) ^ set(b)))
    for n in a:
        x, y = a[n], b[n]
        if torch.is_tensor(x):
            assert torch.is_tensor(y) and x.dtype == y.dtype and x.shape == y.shape, "%s: %s changed its type or shape" % (what, n)
            xb, yb = _bits(x), _bits(y)
            if not torch.equal(xb, yb):
                bad = (xb != yb).reshape(-1).nonzero().reshape(-1)
                raise AssertionError("%s: %s differs in %d of %d elements, first at flat index %d (clean %r, poisoned %r)"
                                     % (what, n, bad.numel(), x.numel(), int(bad[0]), x.reshape(-1)[int(bad[0])].item(),
                                        y.reshape(-1)[int(bad[0])].item()))
        else:
            assert x == y and type(x) is type(y), "%s: %s differs (clean %r, poisoned %r)" % (what, n, x, y)


def _three(monkeypatch, scenario, what):
    """Clean, pattern A, pattern B, in this order; -> the clean result."""
    clean = scenario()
    torch.cuda.synchronize()
    assert _flatten(clean, "", {}), what
    for pattern in poison.PATTERNS:
        with poison.poisoned(monkeypatch, pattern) as sites:
            got = scenario()
            torch.cuda.synchronize()
        assert sites, "%s: no allocation of the package was reached under pattern %s" % (what, pattern)
        _assert_same(clean, got, "%s under pattern %s" % (what, pattern))
    return clean


def _grads(p):
    return {n: t.grad for n, t in p.items() if torch.is_tensor(t) and t.requires_grad}


def _rng_tensor(rng, shape, scale=1.0, grad=False):
    t = _dev((rng.normal(size=shape) * scale).astype(np.float32))
    return t.requires_grad_(True) if grad else t


# ================================================================================================ inference
def _sd(weights, kind):
    if kind not in _CACHE:
        _CACHE[kind] = weights(kind)
    return _CACHE[kind]


def _patches(nq, k, skip):
    key = ("patches", nq, k, skip)
    if key not in _CACHE:
        _CACHE[key] = U.sphere_patches(nq, k, skip=skip)
    return _CACHE[key].to(U.dev())


def _fn_model(weights):
    import sapcu_amd
    fn = sapcu_amd.ImprovedSNNNormalEstimation(**FN_KW)
    fn.load_state_dict(_sd(weights, "fn"), strict=True)
    return fn.to(U.dev())


def _fd_model(weights):
    import sapcu_amd
    fd = sapcu_amd.EnhancedSNNDistanceEstimation(**FD_KW)
    fd.load_state_dict(_sd(weights, "fd"), strict=True)
    return fd.to(U.dev())


_expect("test_fn_inference")


def test_fn_inference(weights, monkeypatch):
    """5 patches of 48 points and 1 of 12 (min(k, N) engages in all three blocks), both cache modes, the cached tables, and one
    call with taps and knn_in."""
    p48, p12 = _patches(5, 48, 0), _patches(1, 12, 7)

    def scenario():
        fn = _fn_model(weights)
        out = {}
        for mode in ("fresh", "reference"):
            fn.knn_cache_mode = mode
            fn._knn_cache.clear()
            out[mode] = [fn(p48), fn(p12), fn(p48), fn(p48.view(1, 5, 48, 3)), fn(p48[:0])]
        out["tables"] = [fn.knn_tables(5, 48), fn.knn_tables(1, 12), fn.tiled_knn_tables(5, 48, 2)]
        z = lambda *s: torch.zeros(s, dtype=F32, device=U.dev())
        taps = {"stem": z(5, 48, 64), "block1": z(5, 48, 64), "block2": z(5, 48, 64), "block3": z(5, 48, 64), "pooled": z(5, 640),
                "enc": z(5, 2048), "logits": z(5, 3)}
        out["forced"] = fn(p48, taps=taps, knn_in=torch.cat([t.reshape(-1) for t in fn.knn_tables(5, 48)]))
        out["taps"] = taps
        out["gemm_mode"] = list(fn.gemm_mode())
        return out
    clean = _three(monkeypatch, scenario, "fn inference")
    assert clean["tables"][1][0].shape == (1, 12, 12) and bool(clean["taps"]["enc"].any())
    _done("test_fn_inference")


_expect("test_fd_inference")


def test_fd_inference(weights, monkeypatch):
    """5 patches of 48 points and 3 of 128, once with taps (the neighbour tables it chose among them), once forced on those."""
    p48, p128 = _patches(5, 48, 0), _patches(3, 128, 11)

    def scenario():
        fd = _fd_model(weights)
        out = {}
        for name, x in (("48", p48), ("128", p128)):
            b, m, T = x.shape[0], x.shape[1], FD_KW["time_steps_enc"]
            z = lambda *s: torch.zeros(s, dtype=F32, device=U.dev())
            taps = {"fused0": z(b, m, 64), "spikes": z(T, b, m, 960), "knn": torch.zeros((3, b, m, 32), dtype=I32, device=U.dev()),
                    "pooled": z(T, b, 768), "enc": z(b, 768)}
            out[name] = {"free": fd(x, taps=taps), "taps": taps, "forced": fd(x, knn_force=taps["knn"]), "plain": fd(x)}
        out["4d"] = fd(p48.view(1, 5, 48, 3))
        out["none"] = fd(p48[:0])
        out["gate"] = fd.gate_violations()
        return out
    clean = _three(monkeypatch, scenario, "fd inference")
    assert clean["gate"] == 0 and bool(clean["128"]["taps"]["knn"].any()) and clean["128"]["forced"].shape == (3,)
    _done("test_fd_inference")


# ================================================================================================ generation
_expect("test_generation_helpers", (1, 130))


@pytest.mark.parametrize("b", [1, 130])
def test_generation_helpers(b, monkeypatch):
    from sapcu_amd import generation as gen, testing as T
    cloud = _dev(T.sphere_cloud(1024, 0))
    q = _dev(T.grid_queries(130, 5)[:b])
    rng = np.random.default_rng(b)
    nrm = _dev(rng.normal(size=(b, 3)).astype(np.float32))
    dist = _dev(rng.random(b).astype(np.float32) * 0.01)

    def scenario():
        idx, d, patch = gen.knn_gather(cloud, q, 48, want_dist=True)
        idx2, none_d, none_p = gen.knn_gather(cloud, q, 7, want_patch=False)
        unit = gen.l2_normalize3(nrm)
        return {"idx": idx, "dist": d, "patch": patch, "idx7": idx2, "absent": [none_d, none_p], "unit": unit,
                "rot": gen.gather_rotate(cloud, q, idx, unit), "moved": gen.displace(q, unit, dist)}
    clean = _three(monkeypatch, scenario, "generation helpers, b = %d" % b)
    assert clean["patch"].shape == (b, 48, 3) and clean["absent"] == [None, None]
    _done("test_generation_helpers", b)


_expect("test_grid_knn_and_outlier_statistics")


def test_grid_knn_and_outlier_statistics(monkeypatch):
    """knn_self_grid at n = 5000 on a row range and on an empty one, at n = 31 with an explicit cell size; the outlier statistics
    and keep mask on those distances; the filter on an empty row range."""
    from sapcu_amd import generation as gen
    big = _dev(np.random.default_rng(5).random((5000, 3)))
    small = _dev(np.random.default_rng(6).random((31, 3)))

    def scenario():
        out, info = {}, []
        out["all"] = gen.knn_self_grid(big, 30, info=info)
        out["info"] = list(info)
        out["range"] = gen.knn_self_grid(big, 30, (5000 // 7, 5000 - 5000 // 5), info=info)
        out["empty"] = gen.knn_self_grid(big, 30, (100, 100))
        out["small"] = gen.knn_self_grid(small, 30, cell_size=0.25, info=info)
        out["small_info"] = list(info)
        for name in ("all", "range", "small"):
            mean, sums = gen.outlier_stats_device(out[name][1])
            gm = gen.outlier_global_mean(sums.cpu(), out[name][1].numel())
            out[name + "/stats"] = [mean, sums, gm, gen.outlier_keep_device(mean, gm, 1.5), gen.outlier_keep_device(mean, gm, 0.9)]
        out["filter"] = gen.outlier_filter_device(big, 1.5)
        all_sums = out["all/stats"][1]
        out["filter_empty"] = gen.outlier_filter_device(big, 1.5, (4096, 4096), lambda sums: all_sums)
        out["filter_tail"] = gen.outlier_filter_device(big, 1.5, (4096, 5000), lambda sums: all_sums)
        return out
    clean = _three(monkeypatch, scenario, "grid kNN and outlier statistics")
    assert clean["info"][0] == 1 and clean["empty"][0].shape == (0, 30) and clean["filter_empty"][0].shape == (0,)
    assert torch.equal(clean["filter"][4096:], clean["filter_tail"][0]) and 0 < int(clean["all/stats"][4].sum()) < 5000
    _done("test_grid_knn_and_outlier_statistics")


_expect("test_dense_seeds_and_fps")


def test_dense_seeds_and_fps(monkeypatch):
    """The smallest clouds of tests/test_gpu_seeds.py (one point; seven points that give no seed; 512 points), once more from
    starting sizes that are too small; farthest point sampling at (n, npoint) = (257, 17) and npoint = 0."""
    from sapcu_amd import generation as gen, pipeline, testing as T
    one = T.sphere_cloud(64, 21)[:1] * 0.05 + 0.01
    xyz = _dev(np.random.default_rng(8).normal(size=(257, 3)).astype(np.float32))

    def scenario():
        out = {}
        for name, cloud, cell, kw in (("n1", one, 0.0175, {}), ("tiny7", T.sphere_cloud(7, 3), 0.05, {}), ("sphere512", T.sphere_cloud(512, 11), 0.05, {}),
                                      ("sphere512_grown", T.sphere_cloud(512, 11), 0.05, dict(max_voxels=64, capacity=8))):
            st = []
            out[name] = [gen.dense_seeds_device(cloud, cell, U.dev(), stats=st, **kw), list(st)[:3]]
        out["fps"] = [pipeline.farthest_point_sample_device(xyz, 17), pipeline.farthest_point_sample_device(xyz, 0),
                      pipeline.farthest_point_sample_device(xyz, 257)]
        return out
    clean = _three(monkeypatch, scenario, "dense seeds and FPS")
    assert clean["sphere512"][0].shape[0] > 0 and torch.equal(clean["sphere512"][0], clean["sphere512_grown"][0])
    assert int(clean["fps"][0][0]) == 257 // 2 and clean["fps"][1].shape == (0,)
    _done("test_dense_seeds_and_fps")


_expect("test_whole_upsample")


def test_whole_upsample(weights, monkeypatch):
    """The 2048-point sphere of golden/e2e_upsample.npz, 901 seeds flooded on the device, refined in batches of 129 and 128
    (np.array_split of 901 by 128: `out`, `normals` and `dists` of Generator3D6.refine are filled chunk by chunk, the chunks of one
    shape fused), both outlier filters."""
    import sapcu_amd
    from sapcu_amd import generation as gen, testing as T
    cloud = T.sphere_cloud(2048, 0)
    sizes = {e - s for s, e in gen.split_batches(901, 128)}
    assert sizes == {128, 129}

    def scenario():
        g = sapcu_amd.Generator3D6(_fn_model(weights), _fd_model(weights), U.dev(), k_neighbors=48, dense_spacing=0.03, batch_size=128)
        g.seed_source = "device"
        seeds = g._dense_seeds(cloud)
        with torch.no_grad():
            refined, normals, dists = g.refine(_dev(cloud), seeds)
        filtered, unfiltered = g.upsample_seeds(cloud, seeds, return_unfiltered=True)
        g.outlier_filter_impl = "device"
        return {"seeds": seeds, "refined": refined, "normals": normals, "dists": dists, "filtered": filtered, "unfiltered": unfiltered,
                "keep": g.outlier_filter(_dev(unfiltered)), "whole": g.upsample(cloud[None])}
    clean = _three(monkeypatch, scenario, "whole upsample")
    assert np.array_equal(clean["seeds"].cpu().numpy(), golden("e2e_upsample.npz")["seeds"])
    assert clean["filtered"].shape[0] == int(clean["keep"].sum()) and np.array_equal(clean["whole"], clean["filtered"])
    _done("test_whole_upsample")


# ================================================================================================ fn training ops
def _neuron_raw(rng, ch, eif=False, grad=True):
    base = {"membrane_decay": 0.9, "threshold_adapt": 0.01, "refractory_decay": 0.5, "threshold_base": 1.0}
    if eif:
        base.update({"delta_T": 1.0, "theta_rh": 0.8})
    raw = {n: (v * (1.0 + 0.1 * rng.normal(size=ch))) for n, v in base.items()}
    # thresholds on both sides of zero, as in trained weights: a self-feeding loop whose thresholds are all near 1 is silent after
    # its first step, and silent outputs test little
    raw["threshold_base"] = rng.normal(0.2, 0.5, size=ch)
    return {n: _dev(v.astype(np.float32)).requires_grad_(grad) for n, v in raw.items()}


_expect("test_fn_training_layers", PRECISIONS)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_fn_training_layers(precision, monkeypatch):
    """lif_selfloop_train, conv_bn_lif_train, conv_bn_train and linear_train, forward and backward, 32 -> 96 channels, at 1 row
    (where BatchNorm's train() mode is not involved), 65 and 1025 rows."""
    from sapcu_amd import train

    def scenario():
        out = {}
        with train.gemm_precision(precision):
            for rows in (1, 65, 1025):
                rng = np.random.default_rng(rows)
                x = _rng_tensor(rng, (rows, 32), 1.5, grad=True)
                w = _rng_tensor(rng, (96, 32), 0.3, grad=True)
                vec = [_rng_tensor(rng, (96,), 0.5, grad=True) for _ in range(3)]                    # bias, gamma, beta
                raw32, raw96 = _neuron_raw(rng, 32), _neuron_raw(rng, 96)
                go32, go96 = _rng_tensor(rng, (rows, 32)), _rng_tensor(rng, (rows, 96))
                y = train.lif_selfloop_train(x, *raw32.values(), steps=4)
                y.backward(go32)
                res = {"lif": y, "lif/g": [x.grad.clone()] + list(_grads(raw32).values())}
                x.grad = None
                y = train.linear_train(x, w, vec[0])
                y.backward(go96)
                res.update({"linear": y, "linear/g": [t.grad.clone() for t in (x, w, vec[0])]})
                if rows > 1:
                    for t in [x, w] + vec:
                        t.grad = None
                    run = (torch.zeros(96, device=U.dev()), torch.ones(96, device=U.dev()), torch.zeros((), dtype=I64, device=U.dev()), 0.1)
                    y = train.conv_bn_lif_train(x, w, *vec, *raw96.values(), steps=4, running=run)
                    y.backward(go96)
                    res.update({"cbl": y, "cbl/g": [t.grad.clone() for t in [x, w] + vec] + list(_grads(raw96).values()), "cbl/run": list(run[:3])})
                    for t in [x, w] + vec:
                        t.grad = None
                    run = (torch.zeros(96, device=U.dev()), torch.ones(96, device=U.dev()), None, 0.1)
                    y = train.conv_bn_train(x, w, *vec, running=run)
                    y.backward(go96)
                    res.update({"cb": y, "cb/g": [t.grad.clone() for t in [x, w] + vec], "cb/run": list(run[:2])})
                    xd = x.detach()                                                                  # no data gradient asked for
                    y = train.conv_bn_train(xd, w, *vec)
                    y.backward(go96)
                    res["cb/no_dx"] = [y, w.grad.clone()]
                out[rows] = res
        return out
    clean = _three(monkeypatch, scenario, "fn training layers, %s" % precision)
    assert bool(clean[1025]["lif"].any()) and bool(clean[1025]["cbl"].any()) and bool(clean[65]["cb/g"][0].any())
    _done("test_fn_training_layers", precision)


_expect("test_fn_training_gathers_softmax_and_max", PRECISIONS)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_fn_training_gathers_softmax_and_max(precision, monkeypatch):
    """softmax_agg with and without keep at (b, m, kk, d) = (2, 5, 5, 64) on a neighbour table that leaves points 3 and 4 of every
    patch without an incoming edge; gather_rows grouped and ungrouped with source rows no index points at (the ungrouped backward
    adds with float atomics: integer-valued gradients keep its sums exact in any order); group_max at (3, 7, 96)."""
    from sapcu_amd import train
    b, m, kk, d = 2, 5, 5, 64
    P = b * m

    def scenario():
        with train.gemm_precision(precision):                  # (no GEMM among these ops: the setting must not matter to them)
            return body()

    def body():
        rng = np.random.default_rng(31)
        out = {}
        idx = _dev(rng.integers(0, 3, size=P * kk).astype(np.int32))
        go = _rng_tensor(rng, (P, d))
        for name in ("plain", "keep"):
            a, pe, v = _rng_tensor(rng, (P * kk, d), 2.0, True), _rng_tensor(rng, (P * kk, d), 1.0, True), _rng_tensor(rng, (P, d), 1.0, True)
            keep = train.dropout_keep((P * kk, d), 0.3, U.dev(), torch.Generator(device=U.dev()).manual_seed(3)) if name == "keep" else None
            res = train.softmax_agg(a, pe, v, idx, m, float(8 ** 0.5), keep)
            res.backward(go)
            out[name] = [res, a.grad, pe.grad, v.grad, keep]
        src = _rng_tensor(rng, (P, d), 1.0, True)
        nbr = _dev((rng.integers(0, 3, size=(b, m * kk)) + np.arange(b)[:, None] * m).reshape(-1).astype(np.int64))
        g = train.gather_rows(src, nbr, (m, m * kk))
        g.backward(_rng_tensor(rng, (P * kk, d)))
        out["grouped"] = [g, src.grad.clone()]
        src.grad = None
        loose = _dev(rng.integers(0, 4, size=37).astype(np.int64) * 2)                               # rows 1, 3, 5, 7, 8, 9: never
        g = train.gather_rows(src, loose)
        g.backward(_dev(rng.integers(-3, 4, size=(37, d)).astype(np.float32)))
        out["loose"] = [g, src.grad.clone()]
        x = _dev(((rng.uniform(size=(3 * 7, 96)) > 0.7) * rng.integers(1, 3, (3 * 7, 96))).astype(np.float32)).requires_grad_(True)
        y = train.group_max(x, 7)
        y.backward(_rng_tensor(rng, (3, 96)))
        out["max"] = [y, x.grad]
        out["knn"] = train.inpatch_knn(_rng_tensor(rng, (3, 7, 3)), 5)
        return out
    clean = _three(monkeypatch, scenario, "fn gathers, softmax-aggregate, max, %s" % precision)
    gv = clean["plain"][3].view(b, m, d)
    assert bool(gv[:, :3].any()) and not bool(gv[:, 3:].any())                                       # no edge, no gradient
    assert not bool(clean["loose"][1][1::2].any()) and not bool(clean["grouped"][1].view(b, m, d)[:, 3:].any())
    _done("test_fn_training_gathers_softmax_and_max", precision)


def _fn_training_tensors():
    """Seed-0 training weights of fn at the conftest settings on the device: parameters require gradients, buffers do not."""
    import sapcu_amd
    from sapcu_amd import testing as T
    if "fn_train_sd" not in _CACHE:
        shell = sapcu_amd.ImprovedSNNNormalEstimation(**FN_KW)
        _CACHE["fn_train_sd"] = (T.training_state_dict(shell.state_dict(), 0), {n for n, _ in shell.named_parameters()})
    sd, params = _CACHE["fn_train_sd"]
    return {n: v.to(U.dev()).clone().requires_grad_(n in params) for n, v in sd.items()}


_expect("test_fn_training_block_and_whole_model", PRECISIONS)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_fn_training_block_and_whole_model(precision, monkeypatch):
    """One transformer_block_train and one fn_train_forward + loss + backward on 2 clouds x 12 points, attention and decoder dropout
    on (seeded), the BatchNorm buffers moving."""
    from sapcu_amd import train

    def scenario():
        rng = np.random.default_rng(12)
        out = {}
        pts = _rng_tensor(rng, (2, 12, 3), 0.05)
        gen = torch.Generator(device=U.dev()).manual_seed(5)
        with train.gemm_precision(precision):
            p = _fn_training_tensors()
            blk = {n[len("encoder.trans1."):]: v for n, v in p.items() if n.startswith("encoder.trans1.")}
            feats = _rng_tensor(rng, (2, 12, 64), 1.0, True)
            y = train.transformer_block_train(blk, pts, feats, train.inpatch_knn(pts, 12), momentum=0.1, attn_dropout=0.1, generator=gen)
            y.backward(_rng_tensor(rng, (2, 12, 64)))
            out["block"] = [y, feats.grad, _grads(blk), {n: v for n, v in blk.items() if not v.requires_grad}]
            p = _fn_training_tensors()
            normals = train.fn_train_forward(p, pts, momentum=0.1, attn_dropout=0.1, decoder_dropout=0.1, generator=gen)
            gt = torch.nn.functional.normalize(_rng_tensor(rng, (2, 3)), dim=-1)
            loss, conf = train.angular_loss_with_consistency(normals, gt, pts)
            loss.backward()
            out["model"] = [normals, loss, conf, _grads(p), {n: v for n, v in p.items() if not v.requires_grad}]
        return out
    clean = _three(monkeypatch, scenario, "fn block and whole model, %s" % precision)
    assert bool(torch.isfinite(clean["model"][1])) and all(g is not None and bool(torch.isfinite(g).all()) for g in clean["model"][3].values())
    _done("test_fn_training_block_and_whole_model", precision)


# ================================================================================================ fd training ops
_expect("test_fd_training_ops", [(pr,) + s for pr in PRECISIONS for s in FD_OP_SHAPES])


@pytest.mark.parametrize("P,M,kk,C", FD_OP_SHAPES)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_fd_training_ops(precision, P, M, kk, C, monkeypatch):
    """Forward and backward of every autograd Function of fd_train.py: the neuron step (LIF and EIF, first step and a step from a
    carried state), the edge feature, the fused EdgeConv -> conv -> BatchNorm (its statistics op) -> LeakyReLU -> max with and
    without a neighbour table, the factored EdgeConv, the feature kNN."""
    from sapcu_amd import fd_train, train

    def scenario():
        rng = np.random.default_rng(P * 100 + M)
        out = {}
        rows = P * M
        idx = _dev(rng.integers(0, M, (P, M, kk)).astype(np.int32))
        with train.gemm_precision(precision):
            for kind in ("lif", "eif"):
                raw = _neuron_raw(rng, C, eif=(kind == "eif"))
                x1, x2 = _rng_tensor(rng, (rows, C), 1.5, True), _rng_tensor(rng, (rows, C), 1.5, True)
                s1, state, pre1 = fd_train.neuron_step_train(x1, raw)
                s2, state2, pre2 = fd_train.neuron_step_train(x2, raw, state)
                forced = (_rng_tensor(rng, (rows, C)) > 0).float()
                s3, state3, pre3 = fd_train.neuron_step_train(x2, raw, state, forced)
                ((s1 * _rng_tensor(rng, (rows, C))).sum() + (s2 * _rng_tensor(rng, (rows, C))).sum() + (s3 * _rng_tensor(rng, (rows, C))).sum()).backward()
                out[kind] = [s1, state, pre1, s2, state2, pre2, s3, state3, pre3, x1.grad, x2.grad, _grads(raw)]
            x = _rng_tensor(rng, (rows, C), 1.0, True)
            f = fd_train.edge_feature(x, idx)
            f.backward(_rng_tensor(rng, (rows * kk, 2 * C)))
            out["feature"] = [f, x.grad.clone(), fd_train.edge_feature_forward(x.detach(), idx, 2 * C + 32)]
            for name in ("edge", "pool", "factored"):
                x.grad = None
                cin = C if name == "pool" else 2 * C
                w = _rng_tensor(rng, (64, cin, 1, 1), 0.2, True)
                gamma, beta = _rng_tensor(rng, (64,), 0.5, True), _rng_tensor(rng, (64,), 0.5, True)
                run = (torch.zeros(64, device=U.dev()), torch.ones(64, device=U.dev()), torch.zeros((), dtype=I64, device=U.dev()), 0.1)
                if name == "edge":
                    y = fd_train.conv_bn_lrelu_max(x, w, gamma, beta, group=kk, idx=idx, running=run, reps=2)
                elif name == "pool":
                    y = fd_train.conv_bn_lrelu_max(x, w, gamma, beta, group=M, running=run)
                else:
                    y = fd_train.edgeconv_factored(x, w, gamma, beta, idx, running=run)
                y.backward(_rng_tensor(rng, tuple(y.shape)))
                out[name] = [y, x.grad.clone(), w.grad, gamma.grad, beta.grad, list(run[:3])]
            xd = x.detach()                                                                          # no data gradient asked for
            for name in ("edge", "factored"):
                w = _rng_tensor(rng, (64, 2 * C), 0.2, True)
                gamma, beta = _rng_tensor(rng, (64,), 0.5, True), _rng_tensor(rng, (64,), 0.5, True)
                y = fd_train.conv_bn_lrelu_max(xd, w, gamma, beta, group=kk, idx=idx) if name == "edge" else fd_train.edgeconv_factored(xd, w, gamma, beta, idx)
                y.backward(_rng_tensor(rng, tuple(y.shape)))
                out[name + "/no_dx"] = [y, w.grad, gamma.grad, beta.grad]
            out["knn"] = fd_train.feature_knn((xd > 0).float(), P, M, kk)
        out["bad"] = fd_train.take_bad_index_count()
        return out
    fd_train.take_bad_index_count()
    clean = _three(monkeypatch, scenario, "fd training ops, %s, (P, M, kk, C) = %s" % (precision, (P, M, kk, C)))
    assert clean["bad"] == 0 and bool(clean["eif"][0].any()) and bool(clean["factored"][1].any())
    assert clean["lif"][11]["threshold_adapt"] is None and clean["lif"][11]["membrane_decay"] is not None
    _done("test_fd_training_ops", (precision, P, M, kk, C))


_expect("test_fd_training_whole_model_step")


def test_fd_training_whole_model_step(monkeypatch):
    """The teacher-forced step of tests/test_gpu_fd_train.py at its smaller configuration (A): taps, prediction, loss, gradients,
    buffers."""
    from test_gpu_fd_train import _config, _forced_run
    kw, g, sd, names = _config("A")

    def scenario():
        p, pred, loss, taps, flip, _ = _forced_run(kw, g, sd, names, True)
        return {"pred": pred, "loss": loss, "taps": taps, "flip": flip, "grads": _grads(p), "buffers": {n: v for n, v in p.items() if not v.requires_grad}}
    _three(monkeypatch, scenario, "fd whole-model step")
    _done("test_fd_training_whole_model_step")


# ================================================================================================ trainers
def _fn_run(graphed, steps=2):
    import test_gpu_fn_graph as FN
    from sapcu_amd import fn_trainer
    batches = FN._batches(steps)
    model, opt, tr = FN._fresh()
    step = fn_trainer.GraphedTrainStep(tr, batches[0], warmup=0) if graphed else tr
    out = []
    for b in batches:
        out.append([list(step.train_step(b)), FN._state(model, opt)])
    return out, step


def _fd_run(kind, steps=2):
    import test_gpu_fd_graph as FD
    from sapcu_amd import fd_trainer
    batches = FD._batches(steps)
    model, opt = FD._fresh(dropout=0.1)
    if kind == "amp":
        tr = fd_trainer.AmpTrainer(model, opt, device=U.dev(), grad_clip=0.1, use_amp=True, edgeconv="factored", gradient_accumulation=2)
    else:
        tr = fd_trainer.Trainer(model, opt, device=U.dev(), grad_clip=0.1)
    step = fd_trainer.GraphedTrainStep(tr, batches[0], warmup=0) if kind == "graphed" else tr
    out = []
    for b in batches:
        out.append([list(step.train_step(b)), FD._state(model, opt)])
    return out, step


_expect("test_trainers_eager", ("fn", "fd", "amp"))


@pytest.mark.parametrize("which", ["fn", "fd", "amp"])
def test_trainers_eager(which, monkeypatch):
    """Two steps of fn_trainer.Trainer and of fd_trainer.Trainer; four calls (two optimiser steps: bf16, factored, gradient
    accumulation 2) of fd_trainer.AmpTrainer: losses, parameters, buffers, optimiser state after every call."""
    def scenario():
        torch.manual_seed(0)
        return _fn_run(False)[0] if which == "fn" else _fd_run(which, 4 if which == "amp" else 2)[0]
    clean = _three(monkeypatch, scenario, "%s trainer" % which)
    assert all(r[0][0] is not None for r in clean)
    if which == "amp":
        assert not any(n.startswith("opt/") for n in clean[0][1]) and float(clean[3][1]["opt/distance_decoder.fc_distance.weight/step"]) == 2
    _done("test_trainers_eager", which)


_expect("test_trainers_graphed", ("fn", "fd"))


@pytest.mark.parametrize("which", ["fn", "fd"])
def test_trainers_graphed(which, monkeypatch):
    """GraphedTrainStep(warmup=0) over the fn and the fd trainer: both steps are replays (the fills of the poisoned buffers are
    captured and run again with them; the shadow copies of train_step.py are among them) and equal the clean graphed run — which
    equals the eager run, as tests/test_gpu_fn_graph.py and tests/test_gpu_fd_graph.py require."""
    def scenario():
        torch.manual_seed(0)
        out, step = _fn_run(True) if which == "fn" else _fd_run("graphed")
        assert (step.captures, step.replays, step.eager_fallbacks) == (1, 2, 0)
        return out
    clean = _three(monkeypatch, scenario, "graphed %s step" % which)
    torch.manual_seed(0)
    eager = _fn_run(False)[0] if which == "fn" else _fd_run("fd")[0]
    _assert_same(eager, clean, "graphed %s step against the eager step" % which)
    _done("test_trainers_graphed", which)


# ================================================================================================ dist.py
_expect("test_dist_helpers_on_a_one_rank_group")


def test_dist_helpers_on_a_one_rank_group(tmp_path, monkeypatch):
    """A one-rank gloo group on a FileStore (no network): the padded all-gathers with fewer local rows than the slab (5 of 7: the
    two padding rows come back too), an empty shard, the seed broadcast, upsample_sharded on no seeds."""
    import torch.distributed as td
    from sapcu_amd import dist as D, generation as gen, testing as T

    class Host(object):                                    # what broadcast_seeds and upsample_sharded use of a generator
        device = U.dev()
        model1 = None

        def _dense_seeds(self, data):
            return gen.dense_seeds(data, 0.05)

    td.init_process_group("gloo", store=td.FileStore(str(tmp_path / "store"), 1), rank=0, world_size=1)
    try:
        group = td.group.WORLD
        rows = _dev(np.random.default_rng(2).random((5, 3)))

        def scenario():
            out = {"refined": D.gather_refined(rows, 7, group), "rows": D._all_gather_rows(rows, [7], group),
                   "mask": D._all_gather_rows((rows[:, 0] > 0.5).to(torch.uint8), [7], group), "exact": D._all_gather_rows(rows, [5], group),
                   "none": D.gather_refined(rows[:0], 0, group), "seeds": D.broadcast_seeds(Host(), T.sphere_cloud(512, 11), group)}
            out["sharded"] = list(D.upsample_sharded(Host(), rows, rows[:0], group))
            return out
        clean = _three(monkeypatch, scenario, "dist helpers")
    finally:
        td.destroy_process_group()
    assert torch.equal(clean["refined"][:5], rows) and not bool(clean["refined"][5:].any()) and clean["refined"].shape == (7, 3)
    assert torch.equal(clean["rows"], clean["refined"]) and torch.equal(clean["exact"], rows) and clean["seeds"].shape[0] > 0
    assert clean["sharded"][0].shape == (0, 3) and clean["sharded"][1] == (0, 0)
    _done("test_dist_helpers_on_a_one_rank_group")


# ================================================================================================ the helper on the device
def test_the_fill_reaches_device_buffers_and_runs_again_at_every_replay(monkeypatch):
    """tests/test_poison_host.py on device tensors, and under stream capture: the fill of a buffer allocated inside a captured
    graph is one of the graph's launches, so a replay finds the pattern again where the graph itself wrote afterwards."""
    from sapcu_amd import train
    for pattern in poison.PATTERNS:
        byte = poison.FLOAT_BYTE[pattern]
        with poison.poisoned(monkeypatch, pattern):
            product = train.torch                                  # what the package's own code calls
            f = product.empty((3, 5), dtype=F32, device=U.dev())
            d = product.empty_like(torch.zeros(7, dtype=F64, device=U.dev()))
            i = product.empty((4,), dtype=I32, device=U.dev())
            w = product.empty((9,), dtype=torch.uint8, device=U.dev())
            k = product.empty((6,), dtype=torch.bool, device=U.dev())
            assert bool((f.view(torch.uint8) == byte).all()) and bool((d.view(torch.uint8) == byte).all())
            assert bool((i == poison.INT_VALUE[pattern]).all()) and bool((w == poison.UINT8_VALUE[pattern]).all())
            assert bool((k == poison.BOOL_VALUE[pattern]).all())
            seen = torch.zeros(8, dtype=F32, device=U.dev())
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                buf = product.empty((8,), dtype=F32, device=U.dev())
                seen.copy_(buf)
                buf.zero_()                                        # the graph's own later write to the same block
            for _ in range(2):
                seen.zero_()
                graph.replay()
                torch.cuda.synchronize()
                assert bool((seen.view(torch.uint8) == byte).all()), pattern
            del graph, buf


# ================================================================================================ the sites
def test_every_allocation_site_was_reached_under_both_patterns():
    missing = sorted((name, case) for name, cases in _EXPECTED.items() for case in cases if case not in _RAN.get(name, ()))
    if missing:
        pytest.skip("not every scenario of this module ran to its end (a -k selection, or a failure above): %s" % (missing,))
    assert len(EXEMPT) * 10 <= len(SITES), "EXEMPT holds %d of %d sites: add a scenario, not an exemption" % (len(EXEMPT), len(SITES))
    assert all(isinstance(r, str) and len(r) > 10 for r in EXEMPT.values())
    known = {(f, line) for f, first, last, _ in SITES for line in range(first, last + 1)}
    assert set(EXEMPT) <= known, "EXEMPT names lines that allocate nothing: %s" % sorted(set(EXEMPT) - known)
    for pattern in poison.PATTERNS:
        reached = poison.REACHED[pattern] | set(EXEMPT)
        left = poison.unreached(SITES, reached)
        print("pattern %s: %d of %d sites reached, %d exempt" % (pattern, len(SITES) - len(poison.unreached(SITES, poison.REACHED[pattern])),
                                                               len(SITES), len(EXEMPT)))
        assert not left, "pattern %s never reached %s" % (pattern, ["%s:%d %s" % (f, line, func) for f, line, _, func in left])
        stale = [s for s in EXEMPT if s in poison.REACHED[pattern]]
        assert not stale, "EXEMPT lists sites a scenario does reach: %s" % stale
