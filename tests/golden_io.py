"""Loader for tests/golden/golden_v1.npz (see tests/golden/make_golden.py), and the split storage of the larger fixtures."""
import glob
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "opencl-path-tracer_amd"))
from ptamd import layout as L  # noqa: E402
from ptamd.host import FlatScene  # noqa: E402

_cache = None
PART_BYTES = 900_000  # a fixture larger than this is committed as NAME.partNN pieces (no committed file exceeds 1 MiB)


def load_npz(name):
    """tests/golden/NAME (an .npz): the file itself, or its pieces NAME.part00, NAME.part01, ... joined in memory."""
    path = os.path.join(HERE, "golden", name)
    if os.path.exists(path):
        return np.load(path)
    parts = sorted(glob.glob(glob.escape(path) + ".part[0-9][0-9]"))
    if not parts:
        raise FileNotFoundError(path)
    data = b""
    for part in parts:
        with open(part, "rb") as f:
            data += f.read()
    return np.load(io.BytesIO(data))


def save_npz_split(path, **arrays):
    """np.savez_compressed(path, **arrays), written as path.partNN pieces of at most PART_BYTES (what load_npz reads back)."""
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    data = buf.getvalue()
    for old in glob.glob(glob.escape(path) + ".part[0-9][0-9]") + ([path] if os.path.exists(path) else []):
        os.remove(old)
    for i in range(0, len(data), PART_BYTES):
        with open(f"{path}.part{i // PART_BYTES:02d}", "wb") as f:
            f.write(data[i:i + PART_BYTES])
    return len(data)


def load():
    global _cache
    if _cache is None:
        z = load_npz("golden_v1.npz")
        out = {}
        for k in z.files:
            if "@" in k:
                name, dt = k.split("@")
                dtype = getattr(L, dt)
                out[name] = np.frombuffer(z[k].tobytes(), dtype).copy()
            else:
                out[k] = z[k]
        _cache = out
    return _cache


def flat_scene(g, prefix):
    return FlatScene(g[prefix + "vertices"], g[prefix + "triangles"], g[prefix + "materials"], g[prefix + "sub_nodes"],
                     g[prefix + "lights"], g[prefix + "top_nodes"], int(g[prefix + "top_root"]),
                     int((g[prefix + "top_nodes"]["isLeaf"] != 0).sum()))


def scene_inputs(g, name):
    """(flat, camera, sky, material_textures) of golden scene `name` ('mixed' | 'inst')."""
    p = f"scene_{name}_"
    return flat_scene(g, p), g[p + "camera"][0], g[p + "sky"], g[p + "tex"]
