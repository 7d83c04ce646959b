"""The C ABI's headers against the binding's tables, for every test that needs a header's declarations: the parser, once, and the
list of (header under include/, name of its table in sapcu_amd/_lib.py)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEADERS = (("sapcu.h", "EXPORTS"), ("sapcu_seeds.h", "SEEDS_EXPORTS"), ("sapcu_fd_train.h", "FD_TRAIN_EXPORTS"),
           ("sapcu_fd_edgeconv.h", "FD_EDGECONV_EXPORTS"), ("sapcu_train_step.h", "TRAIN_STEP_EXPORTS"),
           ("sapcu_metrics.h", "METRICS_EXPORTS"), ("sapcu_data.h", "DATA_EXPORTS"), ("sapcu_mesh.h", "MESH_EXPORTS"),
           ("sapcu_surface.h", "SURFACE_EXPORTS"), ("sapcu_sinkhorn.h", "SINKHORN_EXPORTS"), ("sapcu_ray.h", "RAY_EXPORTS"),
           ("sapcu_normals.h", "NORMALS_EXPORTS"))


def header_entry_points(header="sapcu.h"):
    """{name: parameter list} of a header under include/ (comments stripped, every `sapcu_xxx(...);` declaration).  The name is
    lower case, digits and underscores, the stricter of the two patterns the tests used to carry; both gave this mapping for every
    header (tests/test_abi_tables.py holds the looser one against it)."""
    with open(os.path.join(ROOT, "include", header)) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(sapcu_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)}


def parameter_count(params):
    """The number of parameters of a declaration's list; `(void)` declares none."""
    return len([a for a in params.split(",") if a.strip() and a.strip() != "void"])
