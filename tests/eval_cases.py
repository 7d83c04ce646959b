"""The inputs of the evaluation modules (metrics, mesh, ray, normals, sinkhorn, surface, data) that must be refused, and the valid
ones in every accepted form: one table for tests/golden/record_eval_refusals.py (which records what each call raises, and what the
valid calls return) and for the two replay tests, tests/test_eval_inputs_host.py and tests/test_gpu_eval_inputs.py.

Shapes are the smallest that reach every check: clouds of 6 and 7 points, a tetrahedron (4 vertices, 4 faces), batches of b = 2
entries of n = 4 points.  Every coordinate is representable in f32, so the f32 form of an input holds the same numbers.

``cases(dev)``: [(id, thunk)], every thunk one public call with one fault, or two faults in two arguments (which one is reported is
the precedence).  ``dev`` None gives the cases built from numpy arrays and CPU tensors alone; with a device the same cases, plus the
faults as device tensors, plus the functions whose inputs must be device tensors.  ``ok_calls(dev)``: [(id, thunk)] of valid calls
in the forms numpy / tensor / mixed / f32 / noncontig / readonly.  ``outcome`` runs a thunk -> [exception type, message] or [None,
None]; ``flatten`` turns a result into {name: numpy array}.
"""
import numpy as np
import torch

NAN, INF = float("nan"), float("inf")
FORMS = ("numpy", "tensor", "mixed", "f32", "noncontig", "readonly")


class NeedsDevice(Exception):
    """Raised in place of the current device by ``without_device``: the call got past every host check."""


def without_device(monkeypatch_setattr):
    """Make torch.cuda.current_device raise NeedsDevice, through a setattr(obj, name, value) such as monkeypatch.setattr: the host
    part of the record is the same on a machine with a GPU and on one without."""
    def refuse(*a, **k):
        raise NeedsDevice()
    monkeypatch_setattr(torch.cuda, "current_device", refuse)


def outcome(thunk):
    try:
        thunk()
    except NeedsDevice:
        raise
    except Exception as e:                                                    # noqa: BLE001 - the type is what is recorded
        return [type(e).__name__, str(e)]
    return [None, None]


def _f32(a):
    return np.ascontiguousarray(a.astype(np.float32).astype(np.float64))


def fixtures():
    rs = np.random.RandomState(0)
    fx = {"A": _f32(rs.rand(6, 3)), "B": _f32(rs.rand(7, 3)),
          "V": np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float64),
          "F": np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=np.int64)}
    fx["P"] = _f32(fx["A"] * 0.2 + 0.05)                                      # inside the tetrahedron
    fx["D"], fx["D2"], fx["D7"] = _f32(rs.randn(6, 3)), _f32(rs.randn(6, 3)), _f32(rs.randn(7, 3))
    fx["pd"], fx["tm"] = _f32(rs.rand(6)), _f32(rs.rand(6) + 0.5)
    fx["pot"], fx["f"], fx["g"] = _f32(rs.randn(7) * 0.1), _f32(rs.randn(6) * 0.1), _f32(rs.randn(7) * 0.1)
    fx["clouds"] = rs.rand(2, 4, 3).astype(np.float32)
    fx["dense"], fx["cnormals"] = rs.rand(2, 5, 3).astype(np.float32), rs.randn(2, 4, 3).astype(np.float32)
    fx["rotation"] = np.stack([np.eye(3, dtype=np.float32)[[1, 2, 0]], np.eye(3, dtype=np.float32)])
    fx["scale"], fx["jitter"] = (rs.rand(2) + 0.5).astype(np.float32), (rs.randn(2, 4, 3) * 0.01).astype(np.float32)
    fx["u"], fx["r1"], fx["r2"] = rs.rand(2, 4), rs.rand(2, 4).astype(np.float32), rs.rand(2, 4).astype(np.float32)
    fx["g3"], fx["w"] = rs.randn(8, 3), rs.rand(8)
    return fx


def cloud_variants(x, dev):
    """{fault: the [n,3] cloud x with it}"""
    v = {"rank1": x.reshape(-1).copy(), "last2": x[:, :2].copy(), "int": (x * 8).astype(np.int64), "empty": x[:0].copy(),
         "cpu": torch.from_numpy(x.copy())}
    for name, val in (("nan", NAN), ("pinf", INF), ("ninf", -INF)):
        y = x.copy()
        y[1, 2] = val
        v[name] = y
    if dev is not None:
        for k in [k for k in v if k != "cpu"]:
            v[k + "_dev"] = torch.from_numpy(v[k]).to(dev)
    return v


def face_variants(f, dev):
    hi, neg = f.copy(), f.copy()
    hi[2, 1], neg[1, 0] = 4, -1
    v = {"float": f.astype(np.float64), "empty": f[:0].copy(), "high": hi, "neg": neg, "uhigh": hi.astype(np.uint32),
         "rank1": f.reshape(-1).copy(), "last2": f[:, :2].copy(), "cpu": torch.from_numpy(f.copy()), "bool": f.astype(bool)}
    if dev is not None:
        for k in ("float", "empty", "high", "neg", "last2"):
            v[k + "_dev"] = torch.from_numpy(v[k]).to(dev)
    return v


# two faults at once, (fault of the earlier argument, fault of the later one): which is reported is the precedence
PAIRS = (("nan", "rank1"), ("nan", "int"), ("nan", "cpu"), ("nan", "empty"), ("empty", "int"), ("empty", "nan"), ("cpu", "rank1"),
         ("int", "last2"), ("empty", "cpu"))
FACE_AFTER = (("nan", "float"), ("nan", "high"), ("empty", "float"), ("nan", "empty"), ("nan", "cpu"))


def _modules():
    from sapcu_amd import data, mesh, metrics, normals, ray, sinkhorn, surface
    return data, mesh, metrics, normals, ray, sinkhorn, surface


def _generic(out, dev, cid, fn, args, clouds, faces=None, kw=None):
    """One fault per cloud argument (and per faces argument), then two faults in two arguments."""
    kw = kw or {}
    names = [n for n, _ in args]
    base = [v for _, v in args]

    def call(subst):
        a = list(base)
        for name, value in subst.items():
            a[names.index(name)] = value
        return lambda: fn(*a, **kw)

    var = {n: cloud_variants(base[names.index(n)], dev) for n in clouds}
    if faces:
        var[faces] = face_variants(base[names.index(faces)], dev)
    for n in var:
        for fault, value in var[n].items():
            out.append(("%s/%s=%s" % (cid, n, fault), call({n: value})))
    for i, a in enumerate(clouds):
        for b in clouds[i + 1:]:
            for fa, fb in PAIRS:
                out.append(("%s/%s=%s,%s=%s" % (cid, a, fa, b, fb), call({a: var[a][fa], b: var[b][fb]})))
        if faces:                                                             # the faces follow every cloud in every signature
            for fa, ff in FACE_AFTER:
                out.append(("%s/%s=%s,%s=%s" % (cid, a, fa, faces, ff), call({a: var[a][fa], faces: var[faces][ff]})))


def cases(dev):
    data, mesh, metrics, normals, ray, sinkhorn, surface = _modules()
    fx = fixtures()
    A, B, V, F, P, D, D2, D7 = (fx[k] for k in ("A", "B", "V", "F", "P", "D", "D2", "D7"))
    out = []
    add = lambda cid, thunk: out.append((cid, thunk))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    _generic(out, dev, "metrics.nearest", metrics.nearest, [("queries", A), ("cloud", B)], ["queries", "cloud"])
    _generic(out, dev, "metrics.cloud_metrics", metrics.cloud_metrics, [("pred", A), ("gt", B)], ["pred", "gt"])
    _generic(out, dev, "metrics.dataset_metrics", lambda p, g: metrics.dataset_metrics([(p, g), (B, A)]), [("pred", A), ("gt", B)],
             ["pred", "gt"])
    add("metrics.dataset_metrics/none", lambda: metrics.dataset_metrics([]))

    _generic(out, dev, "mesh.point_to_mesh", mesh.point_to_mesh, [("points", P), ("vertices", V), ("faces", F)], ["points", "vertices"],
             "faces")
    _generic(out, dev, "mesh.mesh_metrics", mesh.mesh_metrics, [("pred", P), ("vertices", V), ("faces", F)], ["pred", "vertices"], "faces")
    _generic(out, dev, "mesh.mesh_dataset_metrics", lambda p, v, f: mesh.mesh_dataset_metrics([(p, v, f), (P, V, F)]),
             [("pred", P), ("vertices", V), ("faces", F)], ["pred", "vertices"], "faces")
    add("mesh.mesh_dataset_metrics/none", lambda: mesh.mesh_dataset_metrics([]))
    flat = np.array([[0, 1, 1], [2, 2, 3], [0, 0, 0], [1, 1, 1]], dtype=np.int64)
    add("mesh.mesh_metrics/every_face_flat", lambda: mesh.mesh_metrics(P, V, flat))

    rays = [("origins", P), ("directions", D), ("vertices", V), ("faces", F)]
    _generic(out, dev, "ray.ray_to_mesh", ray.ray_to_mesh, rays, ["origins", "directions", "vertices"], "faces")
    _generic(out, dev, "ray.signed_ray_distance", ray.signed_ray_distance, rays, ["origins", "directions", "vertices"], "faces")
    _generic(out, dev, "ray.ray_metrics", ray.ray_metrics, [("points", P), ("normals", D), ("pred_d", fx["pd"]), ("vertices", V), ("faces", F)],
             ["points", "normals", "vertices"], "faces")
    add("ray.ray_to_mesh/directions=rows", lambda: ray.ray_to_mesh(P, D7, V, F))
    add("ray.ray_to_mesh/directions=rows,vertices=nan", lambda: ray.ray_to_mesh(P, D7, cloud_variants(V, None)["nan"], F))
    tmax = {"rows": fx["tm"][:5], "rank2": fx["tm"].reshape(6, 1), "cpu": torch.from_numpy(fx["tm"].copy()),
            "cpu_int": torch.arange(6), "text": "far"}
    pred = {"rows": fx["pd"][:5], "cpu": torch.from_numpy(fx["pd"].copy()), "rank2": np.stack([fx["pd"], fx["pd"]])}
    if dev is not None:
        tmax.update(rows_dev=up(fx["tm"][:5]), int_dev=torch.arange(6, device=dev), rank2_dev=up(fx["tm"].reshape(6, 1)))
        pred.update(rows_dev=up(fx["pd"][:5]))
    for fault, t in tmax.items():
        add("ray.ray_to_mesh/t_max=%s" % fault, lambda t=t: ray.ray_to_mesh(P, D, V, F, t_max=t))
        add("ray.signed_ray_distance/t_max=%s" % fault, lambda t=t: ray.signed_ray_distance(P, D, V, F, t_max=t))
        add("ray.ray_to_mesh/directions=nan,faces=high,t_max=%s" % fault,
            lambda t=t: ray.ray_to_mesh(P, D7, V, face_variants(F, None)["high"], t_max=t))
    for fault, t in pred.items():
        add("ray.ray_metrics/pred_d=%s" % fault, lambda t=t: ray.ray_metrics(P, D, t, V, F))
        add("ray.ray_metrics/pred_d=%s,points=nan" % fault, lambda t=t: ray.ray_metrics(cloud_variants(P, None)["nan"], D, t, V, F))
    add("ray.ray_metrics/no_hit", lambda: ray.ray_metrics(P + 5.0, np.ones((6, 3)), fx["pd"], V, F))
    add("ray.is_watertight/float", lambda: ray.is_watertight(F.astype(np.float64)))
    add("ray.is_watertight/last2", lambda: ray.is_watertight(F[:, :2]))
    add("ray.sample_fd_rays/tables", lambda: ray.sample_fd_rays(None, 0, None, None, None, None, None))

    _generic(out, dev, "normals.pca_normals", lambda p: normals.pca_normals(p, k=4), [("points", A)], ["points"])
    add("normals.pca_normals/n=2", lambda: normals.pca_normals(A[:2], k=4))
    add("normals.pca_normals/k=2", lambda: normals.pca_normals(A, k=2))
    add("normals.pca_normals/k=2,points=nan", lambda: normals.pca_normals(cloud_variants(A, None)["nan"], k=2))
    add("normals.pca_normals/k=70", lambda: normals.pca_normals(np.zeros((70, 3)), k=70))
    add("normals.pca_normals/chunk_rows=0", lambda: normals.pca_normals(A, k=4, chunk_rows=0))
    add("normals.pca_normals/viewpoint=2", lambda: normals.pca_normals(A, k=4, viewpoint=(0.0, 1.0)))
    add("normals.pca_normals/viewpoint=nan,points=nan", lambda: normals.pca_normals(cloud_variants(A, None)["nan"], k=4, viewpoint=(0, NAN, 0)))
    _generic(out, dev, "normals.normal_angles", normals.normal_angles, [("a", D), ("b", D2)], ["a", "b"])
    add("normals.normal_angles/rows", lambda: normals.normal_angles(D, D7))
    add("normals.normal_angles/clamp_eps", lambda: normals.normal_angles(D, D2, clamp_eps=2.0))
    add("normals.normal_angles/rows,clamp_eps", lambda: normals.normal_angles(D, D7, clamp_eps=2.0))
    _generic(out, dev, "normals.normal_metrics", normals.normal_metrics, [("pred_normals", D), ("gt_normals", D2)], ["pred_normals", "gt_normals"])
    _generic(out, dev, "normals.normal_metrics+points", normals.normal_metrics,
             [("pred_normals", D), ("gt_normals", D7), ("pred_points", A), ("gt_points", B)],
             ["pred_normals", "gt_normals", "pred_points", "gt_points"])
    add("normals.normal_metrics/rows", lambda: normals.normal_metrics(D, D7))
    add("normals.normal_metrics/one_cloud", lambda: normals.normal_metrics(D, D2, pred_points=A))
    add("normals.normal_metrics+points/rows", lambda: normals.normal_metrics(D, D7, B, A))
    add("normals.normal_metrics+points/rows,gt_points=nan", lambda: normals.normal_metrics(D, D7, B, cloud_variants(A, None)["nan"]))
    _generic(out, dev, "normals.cloud_normal_metrics", lambda p, g, n: normals.cloud_normal_metrics(p, g, n, k=4),
             [("pred_points", A), ("gt_points", B), ("gt_normals", D7)], ["pred_points", "gt_points", "gt_normals"])

    _generic(out, dev, "sinkhorn.sinkhorn_potentials", lambda x, y: sinkhorn.sinkhorn_potentials(x, y, iters=3), [("x", A), ("y", B)],
             ["x", "y"])
    _generic(out, dev, "sinkhorn.sinkhorn_potentials(x)", lambda x: sinkhorn.sinkhorn_potentials(x, iters=3), [("x", A)], ["x"])
    _generic(out, dev, "sinkhorn.sinkhorn_metrics", lambda p, g: sinkhorn.sinkhorn_metrics(p, g, iters=3), [("pred", A), ("gt", B)],
             ["pred", "gt"])
    _generic(out, dev, "sinkhorn.dataset_sinkhorn", lambda p, g: sinkhorn.dataset_sinkhorn([(p, g)], iters=3), [("pred", A), ("gt", B)],
             ["pred", "gt"])
    bad = cloud_variants(A, None)["nan"]
    for name, kw in (("p=3", dict(p=3)), ("blur=0", dict(blur=0.0)), ("iters=-1", dict(iters=-1)), ("scaling=1", dict(scaling=1.0)),
                     ("downsample_gt=0", dict(downsample_gt=0)), ("downsample_gt=9", dict(downsample_gt=9))):
        add("sinkhorn.sinkhorn_metrics/%s" % name, lambda kw=kw: sinkhorn.sinkhorn_metrics(A, B, **kw))
        add("sinkhorn.sinkhorn_metrics/%s,pred=nan" % name, lambda kw=kw: sinkhorn.sinkhorn_metrics(bad, B, **kw))
        add("sinkhorn.sinkhorn_metrics/%s,gt=int" % name, lambda kw=kw: sinkhorn.sinkhorn_metrics(A, (B * 8).astype(np.int64), **kw))
    add("sinkhorn.dataset_sinkhorn/none", lambda: sinkhorn.dataset_sinkhorn([]))
    add("sinkhorn.softmin/p=3,x=cpu", lambda: sinkhorn.softmin(cloud_variants(A, None)["cpu"], B, fx["pot"], 3, 0.01))
    add("sinkhorn.softmin/eps=0,x=rank1", lambda: sinkhorn.softmin(A.reshape(-1), B, fx["pot"], 2, 0.0))
    add("sinkhorn.plan_stats/p=3,x=cpu", lambda: sinkhorn.plan_stats(cloud_variants(A, None)["cpu"], B, None, None, 3, 0.01))

    tet32 = (V.astype(np.float32), F)
    for name, pair in (("v_rank1", (V.reshape(-1), F)), ("f_last2", (V, F[:, :2])), ("v_int", (V.astype(np.int64), F)),
                       ("f_float", (V, F.astype(np.float64))), ("v_empty", (V[:0], F)), ("f_empty", (V, F[:0])),
                       ("f_high", (V, face_variants(F, None)["high"])), ("f_neg", (V, face_variants(F, None)["neg"])),
                       ("v_int,f_float", (V.astype(np.int64), F.astype(np.float64))), ("flat", (V, flat)),
                       ("cpu_tensors_flat", (torch.from_numpy(V.copy()), torch.from_numpy(flat.copy())))):
        add("surface.build_surface_tables/%s" % name, lambda pair=pair: surface.build_surface_tables([tet32, pair]))
        add("surface.build_surface_tables/%s,device=cpu" % name, lambda pair=pair: surface.build_surface_tables([tet32, pair], device="cpu"))
    add("surface.build_surface_tables/none", lambda: surface.build_surface_tables([]))
    add("surface.build_surface_tables/names", lambda: surface.build_surface_tables([tet32], names=["a", "b"]))
    add("surface.build_surface_tables/named", lambda: surface.build_surface_tables([tet32, (V, F[:0])], names=["a", "b"]))
    add("surface.sample_surface/tables", lambda: surface.sample_surface(None, None, 4, None, None, None))

    cl = torch.from_numpy(fx["clouds"])
    add("data.build_patches/clouds=numpy", lambda: data.build_patches(fx["clouds"], torch.zeros(2, dtype=torch.int64), 3))
    add("data.build_patches/clouds=cpu", lambda: data.build_patches(cl, torch.zeros(2, dtype=torch.int64), 3))
    if dev is None:
        return out

    # ------------------------------------------------------------------------------------------- device tensors required from here on
    pot, f, g = up(fx["pot"]), up(fx["f"]), up(fx["g"])
    _generic(out, dev, "sinkhorn.softmin", lambda x, y: sinkhorn.softmin(x, y, pot, 2, 0.01), [("x", A), ("y", B)], ["x", "y"])
    _generic(out, dev, "sinkhorn.plan_stats", lambda x, y: sinkhorn.plan_stats(x, y, f, g, 2, 0.01), [("x", A), ("y", B)], ["x", "y"])
    for fault, t in (("rows", pot[:6]), ("rank2", pot.reshape(7, 1)), ("cpu", pot.cpu()), ("numpy", fx["pot"]), ("scalar", pot[0])):
        add("sinkhorn.softmin/pot_y=%s" % fault, lambda t=t: sinkhorn.softmin(A, B, t, 2, 0.01))
        add("sinkhorn.softmin/pot_y=%s,x=empty" % fault, lambda t=t: sinkhorn.softmin(A[:0], B, t, 2, 0.01))
    for fault, (tf, tg) in (("f_rows", (f[:5], g)), ("g_rows", (f, g[:6])), ("swapped", (g, f)), ("f_rank2", (f.reshape(6, 1), g))):
        add("sinkhorn.plan_stats/%s" % fault, lambda tf=tf, tg=tg: sinkhorn.plan_stats(A, B, tf, tg, 2, 0.01))
        add("sinkhorn.plan_stats/%s,x=empty" % fault, lambda tf=tf, tg=tg: sinkhorn.plan_stats(A[:0], B, tf, tg, 2, 0.01))

    pts, idx = up(A), torch.tensor([[0, 1, 2, 3], [1, 0, 2, 5], [2, 1, 0, 4]], dtype=torch.int64, device=dev)
    bad_idx, neg_idx = idx.clone(), idx.clone()
    bad_idx[1, 2], neg_idx[0, 3] = 6, -1
    for fault, (p_, i_) in (("points=f32", (pts.float(), idx)), ("points=cpu", (pts.cpu(), idx)), ("points=numpy", (A, idx)),
                            ("points=empty", (pts[:0], idx)), ("idx=int32", (pts, idx.int())), ("idx=cpu", (pts, idx.cpu())),
                            ("idx=k2", (pts, idx[:, :2].contiguous())), ("idx=noncontig", (pts, idx[:, :3])), ("idx=high", (pts, bad_idx)),
                            ("idx=neg", (pts, neg_idx)), ("points=noncontig", (torch.stack([pts, pts], -1)[..., 0], idx))):
        add("normals.normals_from_neighbours/%s" % fault, lambda p_=p_, i_=i_: normals.normals_from_neighbours(p_, i_))
    add("normals.normals_from_neighbours/viewpoint", lambda: normals.normals_from_neighbours(pts, idx, viewpoint=(0, INF, 0)))

    tables = surface.build_surface_tables([tet32, (V.astype(np.float32) * 2, F)], device=dev)
    mi, u, r1, r2 = torch.tensor([1, 0], dtype=torch.int64, device=dev), up(fx["u"]), up(fx["r1"]), up(fx["r2"])
    sargs = {"mesh_idx": mi, "u": u, "r1": r1, "r2": r2}
    sfaults = {"mesh_idx": {"numpy": mi.cpu().numpy(), "cpu": mi.cpu(), "rank2": mi.reshape(2, 1), "float": mi.double(),
                            "high": torch.tensor([1, 2], dtype=torch.int64, device=dev), "neg": torch.tensor([-1, -3], dtype=torch.int64, device=dev)},
               "u": {"numpy": fx["u"], "cpu": u.cpu(), "rows": u[:1], "cols": u[:, :3], "rank1": u.reshape(-1), "int": (u * 8).long()},
               "r1": {"numpy": fx["r1"], "cpu": r1.cpu(), "cols": r1[:, :3], "int": (r1 * 8).int()},
               "r2": {"list": [[0.0] * 4] * 2, "cpu": r2.cpu(), "rank3": r2.reshape(2, 4, 1), "int": (r2 * 8).long()}}

    def sample(n=4, validate=True, **subst):
        a = dict(sargs, **subst)
        return lambda: surface.sample_surface(tables, a["mesh_idx"], n, a["u"], a["r1"], a["r2"], validate=validate)

    for name, faults in sfaults.items():
        for fault, t in faults.items():
            add("surface.sample_surface/%s=%s" % (name, fault), sample(**{name: t}))
    add("surface.sample_surface/n=0", sample(n=0))
    add("surface.sample_surface/n=4097,u=cpu", sample(n=4097, u=u.cpu()))
    add("surface.sample_surface/mesh_idx=high,u=cpu", sample(mesh_idx=sfaults["mesh_idx"]["high"], u=u.cpu()))
    add("surface.sample_surface/u=cols,r1=cpu", sample(u=u[:, :3], r1=r1.cpu()))
    add("surface.sample_surface/u=int,r1=cols", sample(u=(u * 8).long(), r1=r1[:, :3]))
    add("surface.sample_surface/mesh_idx=cpu,u=numpy", sample(mesh_idx=mi.cpu(), u=fx["u"]))

    g3, w = up(fx["g3"]), up(fx["w"])
    u8, r18, r28 = u.reshape(-1), r1.reshape(-1), r2.reshape(-1)
    open_tables = surface.build_surface_tables([(V.astype(np.float32), F[:3])], device=dev)
    fd = lambda m=0, t=tables, **s: (lambda: ray.sample_fd_rays(t, m, s.get("u", u8), s.get("r1", r18), s.get("r2", r28), s.get("g", g3),
                                                               s.get("w", w)))
    add("ray.sample_fd_rays/mesh_idx=2", fd(m=2))
    add("ray.sample_fd_rays/mesh_idx=-1", fd(m=-1))
    add("ray.sample_fd_rays/open", fd(t=open_tables))
    add("ray.sample_fd_rays/open,u=cpu", fd(t=open_tables, u=u8.cpu()))
    for name, faults in (("u", {"numpy": fx["u"].reshape(-1), "cpu": u8.cpu(), "int": (u8 * 8).long(), "rows": u8[:7], "rank2": u}),
                         ("r1", {"cpu": r18.cpu(), "int": (r18 * 8).long(), "rows": r18[:7]}),
                         ("r2", {"numpy": fx["r2"].reshape(-1), "rank2": r2}),
                         ("g", {"numpy": fx["g3"], "cpu": g3.cpu(), "int": g3.long(), "rows": g3[:7], "last2": g3[:, :2], "rank1": g3.reshape(-1)}),
                         ("w", {"cpu": w.cpu(), "int": (w * 8).long(), "rows": w[:7], "rank2": w.reshape(8, 1)})):
        for fault, t in faults.items():
            add("ray.sample_fd_rays/%s=%s" % (name, fault), fd(**{name: t}))
    add("ray.sample_fd_rays/u=rows,g=cpu", fd(u=u8[:7], g=g3.cpu()))
    add("ray.sample_fd_rays/r1=int,w=numpy", fd(r1=(r18 * 8).long(), w=fx["w"]))

    pargs = {"clouds": up(fx["clouds"]), "sample_idx": torch.tensor([1, 0], dtype=torch.int64, device=dev), "dense": up(fx["dense"]),
             "normals": up(fx["cnormals"]), "rotation": up(fx["rotation"]), "scale": up(fx["scale"]), "jitter": up(fx["jitter"]),
             "centres": torch.tensor([[0, 3], [2, 2]], dtype=torch.int32, device=dev)}
    c = pargs
    pfaults = {"clouds": {"rank2": c["clouds"][0], "last2": c["clouds"][..., :2], "int": (c["clouds"] * 8).int(), "none": c["clouds"][:0],
                          "n=0": c["clouds"][:, :0], "n=4097": torch.zeros((1, 4097, 3), device=dev), "list": fx["clouds"].tolist()},
               "sample_idx": {"numpy": np.array([1, 0]), "cpu": c["sample_idx"].cpu(), "float": c["sample_idx"].float(),
                              "rank2": c["sample_idx"].reshape(2, 1), "high": torch.tensor([2, 0], dtype=torch.int64, device=dev),
                              "neg": torch.tensor([-1, -1], dtype=torch.int64, device=dev)},
               "dense": {"numpy": fx["dense"], "cpu": c["dense"].cpu(), "samples": c["dense"][:1], "last2": c["dense"][..., :2],
                         "g=0": c["dense"][:, :0], "int": (c["dense"] * 8).long()},
               "normals": {"cpu": c["normals"].cpu(), "points": c["normals"][:, :3], "int": c["normals"].long(), "rank2": c["normals"][0]},
               "rotation": {"cpu": c["rotation"].cpu(), "rows": c["rotation"][:1], "2x2": c["rotation"][:, :2, :2], "int": c["rotation"].int()},
               "scale": {"numpy": fx["scale"], "cpu": c["scale"].cpu(), "rows": c["scale"][:1], "rank2": c["scale"].reshape(2, 1),
                         "int": c["scale"].long()},
               "jitter": {"cpu": c["jitter"].cpu(), "points": c["jitter"][:, :3], "rows": c["jitter"][:1], "int": c["jitter"].int()},
               "centres": {"numpy": c["centres"].cpu().numpy(), "cpu": c["centres"].cpu(), "rows": c["centres"][:1], "rank1": c["centres"][0],
                           "float": c["centres"].float(), "none": c["centres"][:, :0],
                           "high": torch.tensor([[0, 4], [1, 1]], dtype=torch.int32, device=dev),
                           "neg": torch.tensor([[0, -1], [-2, 1]], dtype=torch.int32, device=dev)}}

    def patches(k=3, validate=True, **subst):
        a = dict(pargs, **subst)
        return lambda: data.build_patches(a["clouds"], a["sample_idx"], k, dense=a["dense"], normals=a["normals"], rotation=a["rotation"],
                                          scale=a["scale"], jitter=a["jitter"], centres=a["centres"], validate=validate)

    for name, faults in pfaults.items():
        for fault, t in faults.items():
            add("data.build_patches/%s=%s" % (name, fault), patches(**{name: t}))
    add("data.build_patches/k=0", patches(k=0))
    add("data.build_patches/k=0,centres=none", patches(k=0, centres=pfaults["centres"]["none"]))
    add("data.build_patches/sample_idx=high,centres=high", patches(sample_idx=pfaults["sample_idx"]["high"], centres=pfaults["centres"]["high"]))
    add("data.build_patches/sample_idx=high,centres=cpu", patches(sample_idx=pfaults["sample_idx"]["high"], centres=c["centres"].cpu()))
    add("data.build_patches/dense=samples,normals=cpu", patches(dense=c["dense"][:1], normals=c["normals"].cpu()))
    add("data.build_patches/dense=g=0,normals=int", patches(dense=c["dense"][:, :0], normals=c["normals"].long()))
    add("data.build_patches/clouds=last2,dense=cpu", patches(clouds=c["clouds"][..., :2], dense=c["dense"].cpu()))
    add("data.build_patches/rotation=int,scale=rows", patches(rotation=c["rotation"].int(), scale=c["scale"][:1]))
    add("data.build_patches/jitter=rows,centres=numpy", patches(jitter=c["jitter"][:1], centres=c["centres"].cpu().numpy()))
    return out


# ------------------------------------------------------------------------------------------------------------ valid calls
def _form(x, form, dev, i):
    """The i-th floating input of a call, a numpy f64 array, in one of FORMS."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if form == "numpy":
        return x
    if form == "tensor":
        return t(x)
    if form == "mixed":
        return t(x) if i % 2 == 0 else x
    if form == "f32":
        return x.astype(np.float32) if i % 2 == 0 else t(x).float()
    if form == "noncontig":
        if i % 2 == 0:
            return np.stack([x, x], axis=-1)[..., 0]
        return torch.stack([t(x), t(x)], dim=-1)[..., 0]
    y = x.copy()
    y.setflags(write=False)
    return y


def _device_form(v, form):
    """A device-tensor input in the forms that keep it one: as it is, the other float width, or strided."""
    if not torch.is_tensor(v) or form == "tensor":
        return v
    if form == "f32":
        return v.to(torch.float64 if v.dtype == torch.float32 else torch.float32) if v.dtype.is_floating_point else v.to(
            torch.int32 if v.dtype == torch.int64 else torch.int64)
    return torch.stack([v, v], dim=-1)[..., 0]


def ok_calls(dev):
    data, mesh, metrics, normals, ray, sinkhorn, surface = _modules()
    fx = fixtures()
    A, B, V, F, P, D, D2, D7 = (fx[k] for k in ("A", "B", "V", "F", "P", "D", "D2", "D7"))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = []
    pot, f, g = up(fx["pot"]), up(fx["f"]), up(fx["g"])
    host = (("metrics.nearest", metrics.nearest, (A, B)), ("metrics.cloud_metrics", metrics.cloud_metrics, (A, B)),
            ("metrics.dataset_metrics", lambda a, b: metrics.dataset_metrics([(a, b), (b, a)]), (A, B)),
            ("mesh.point_to_mesh", mesh.point_to_mesh, (P, V, F)), ("mesh.mesh_metrics", mesh.mesh_metrics, (P, V, F)),
            ("mesh.mesh_dataset_metrics", lambda p, v, fc: mesh.mesh_dataset_metrics([(p, v, fc), (p * 0.5, v, fc)]), (P, V, F)),
            ("ray.ray_to_mesh", ray.ray_to_mesh, (P, D, V, F)),
            ("ray.ray_to_mesh(t_max)", lambda o, d, t, v, fc: ray.ray_to_mesh(o, d, v, fc, t_max=t), (P, D, fx["tm"] * 0.2, V, F)),
            ("ray.ray_to_mesh(t_max=0.3)", lambda o, d, v, fc: ray.ray_to_mesh(o, d, v, fc, t_max=0.3), (P, D, V, F)),
            ("ray.signed_ray_distance", ray.signed_ray_distance, (P, D, V, F)),
            ("ray.ray_metrics", ray.ray_metrics, (P, D, fx["pd"], V, F)),
            ("normals.pca_normals", lambda p: normals.pca_normals(p, k=4, return_evals=True), (A,)),
            ("normals.pca_normals(view)", lambda p: normals.pca_normals(p, k=5, viewpoint=(0.0, 0.0, 3.0), chunk_rows=4), (B,)),
            ("normals.normal_angles", lambda a, b: normals.normal_angles(a, b, return_cos=True), (D, D2)),
            ("normals.normal_metrics", normals.normal_metrics, (D, D2)),
            ("normals.normal_metrics+points", lambda a, b, p, q: normals.normal_metrics(a, b, p, q, oriented=True, clamp_eps=1e-6), (D, D7, A, B)),
            ("normals.cloud_normal_metrics", lambda p, q, n: normals.cloud_normal_metrics(p, q, n, k=4), (A, B, D7)),
            ("sinkhorn.softmin", lambda x, y: sinkhorn.softmin(x, y, pot, 2, 0.01), (A, B)),
            ("sinkhorn.plan_stats", lambda x, y: sinkhorn.plan_stats(x, y, f, g, 1, 0.1), (A, B)),
            ("sinkhorn.sinkhorn_potentials", lambda x, y: sinkhorn.sinkhorn_potentials(x, y, blur=0.3, iters=3, scaling=0.5), (A, B)),
            ("sinkhorn.sinkhorn_potentials(x)", lambda x: sinkhorn.sinkhorn_potentials(x, blur=0.3, iters=3), (A,)),
            ("sinkhorn.sinkhorn_metrics", lambda a, b: sinkhorn.sinkhorn_metrics(a, b, blur=0.3, iters=3, scaling=0.5, downsample_gt=5), (A, B)),
            ("sinkhorn.dataset_sinkhorn", lambda a, b: sinkhorn.dataset_sinkhorn([(a, b), (b, a)], p=1, blur=0.3, iters=2), (A, B)))
    for cid, fn, args in host:
        for form in FORMS:
            conv, i = [], 0
            for a in args:
                if a.dtype.kind == "f":
                    conv.append(_form(a, form, dev, i))
                    i += 1
                else:
                    conv.append(up(a) if form == "tensor" else a.astype(np.int32) if form == "f32" else a)
            out.append(("%s/%s" % (cid, form), lambda fn=fn, conv=conv: fn(*conv)))

    tet32 = (V.astype(np.float32), F)
    out.append(("surface.build_surface_tables/numpy", lambda: _tables(surface.build_surface_tables([tet32, (V * 2, F.astype(np.uint16))], device=dev))))
    out.append(("surface.build_surface_tables/tensor", lambda: _tables(surface.build_surface_tables([(up(V), up(F)), (torch.from_numpy(V * 2), F)]))))
    tables = surface.build_surface_tables([tet32, (V.astype(np.float32) * 2, F)], device=dev)
    pts, idx = up(A), torch.tensor([[0, 1, 2, 3], [1, 0, 2, 5], [2, 1, 0, 4]], dtype=torch.int64, device=dev)
    out.append(("normals.normals_from_neighbours/tensor", lambda: normals.normals_from_neighbours(pts, idx, viewpoint=(1.0, 2.0, 3.0), return_evals=True)))
    mi, u, r1, r2 = torch.tensor([1, 0], dtype=torch.int64, device=dev), up(fx["u"]), up(fx["r1"]), up(fx["r2"])
    g3, w = up(fx["g3"]), up(fx["w"])
    pargs = {"dense": up(fx["dense"]), "normals": up(fx["cnormals"]), "rotation": up(fx["rotation"]), "scale": up(fx["scale"]),
             "jitter": up(fx["jitter"]), "centres": torch.tensor([[0, 3], [2, 2]], dtype=torch.int32, device=dev)}
    clouds, sidx = up(fx["clouds"]), torch.tensor([1, 0], dtype=torch.int64, device=dev)
    for form in ("tensor", "f32", "noncontig"):
        c = lambda v, form=form: _device_form(v, form)
        out.append(("surface.sample_surface/%s" % form, lambda c=c: surface.sample_surface(tables, c(mi), 4, c(u), c(r1), c(r2))))
        out.append(("ray.sample_fd_rays/%s" % form, lambda c=c: ray.sample_fd_rays(tables, 1, c(u.reshape(-1)), c(r1.reshape(-1)), c(r2.reshape(-1)),
                                                                                  c(g3), c(w))))
        out.append(("data.build_patches/%s" % form, lambda c=c: data.build_patches(c(clouds), c(sidx), 3, **{k: c(v) for k, v in pargs.items()})))
        out.append(("data.build_patches(plain)/%s" % form, lambda c=c: data.build_patches(c(clouds), c(sidx), 9)))
    return out


def _tables(t):
    return {k: getattr(t, k) for k in ("vertices", "vert_off", "faces", "face_off", "face_normals", "cdf", "area_sum", "prob_sum")}


def flatten(result, prefix=""):
    """{name: numpy array} of what a call returned: tensors, numbers, None (left out), and tuples, lists and dicts of them."""
    if result is None:
        return {}
    if torch.is_tensor(result):
        return {prefix or "0": result.detach().cpu().numpy()}
    if isinstance(result, dict):
        items = [(str(k), v) for k, v in result.items()]
    elif isinstance(result, (tuple, list)):
        items = [(str(i), v) for i, v in enumerate(result)]
    else:
        return {prefix or "0": np.asarray(result)}
    out = {}
    for k, v in items:
        out.update(flatten(v, prefix + "." + k if prefix else k))
    return out


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
