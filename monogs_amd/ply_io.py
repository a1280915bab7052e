"""Map persistence: the Gaussian map as a PLY file.

On-disk format of the reference's ``GaussianModel.save_ply`` / ``load_ply``
(/root/reference/gaussian_splatting/scene/gaussian_model.py:467-520,537-640): one ``vertex`` element of float32
properties ``x y z nx ny nz f_dc_0.. opacity scale_0.. rot_0..3`` (normals are zeros; this fork keeps raw RGB
in f_dc and writes no f_rest), binary little-endian as plyfile writes it.  plyfile is not installed here, so the
file is written and parsed directly with numpy; a file written by the reference loads here and vice versa.
Values are the RAW parameters (pre-activation opacity / scaling, un-normalised rotation), as in the reference.
Parity unpinned: the reference holds no PLY fixture.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional

import numpy as np
import torch


def attribute_names(n_dc: int, n_scale: int, n_rot: int = 4, n_obj: int = 0) -> List[str]:
    names = ["x", "y", "z", "nx", "ny", "nz"]
    names += [f"f_dc_{i}" for i in range(n_dc)]
    names += ["opacity"]
    names += [f"scale_{i}" for i in range(n_scale)]
    names += [f"rot_{i}" for i in range(n_rot)]
    names += [f"obj_prob_{i}" for i in range(n_obj)]
    return names


def save_ply(path: str, xyz: torch.Tensor, f_dc: torch.Tensor, opacity: torch.Tensor, scaling: torch.Tensor,
             rotation: torch.Tensor, obj_prob: Optional[torch.Tensor] = None) -> None:
    """xyz [P,3], f_dc [P,3] (or [P,C,1]/[P,1,C] as the reference stores it), opacity [P,1], scaling [P,1|3], rotation [P,4].
    ``obj_prob`` [P,K]: the map's RAW object rows, written as ``obj_prob_0..K-1`` after ``rot_*`` (the reference's TODO at
    gaussian_model.py:505; a reader that does not know them skips them by name); None: the file of a map without the layer."""
    def cpu(t):
        t = t.detach().to("cpu", torch.float32)
        return t.reshape(t.shape[0], int(np.prod(t.shape[1:]))).numpy()

    xyz_, dc, op, sc, rot = cpu(xyz), cpu(f_dc), cpu(opacity), cpu(scaling), cpu(rotation)
    P = xyz_.shape[0]
    obj = [] if obj_prob is None else [cpu(obj_prob)]
    if obj and obj[0].shape[0] != P:
        raise ValueError(f"obj_prob has {obj[0].shape[0]} rows, the map {P}")
    names = attribute_names(dc.shape[1], sc.shape[1], rot.shape[1], obj[0].shape[1] if obj else 0)
    table = np.concatenate([xyz_, np.zeros_like(xyz_), dc, op, sc, rot] + obj, axis=1).astype("<f4")
    assert table.shape == (P, len(names))
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % P
    header += "".join(f"property float {n}\n" for n in names) + "end_header\n"
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(table.tobytes())


_PLY_TYPES = {"float": "f4", "float32": "f4", "double": "f8", "float64": "f8", "uchar": "u1", "uint8": "u1",
              "char": "i1", "int8": "i1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4"}


def read_vertex_table(path: str) -> Dict[str, np.ndarray]:
    """Every scalar property of the ``vertex`` element (binary little/big endian or ascii)."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        fmt, n, props, in_vertex = None, 0, [], False
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: truncated header")
            tok = line.decode("ascii").split()
            if not tok or tok[0] == "comment":
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                in_vertex = tok[1] == "vertex"
                if in_vertex:
                    n = int(tok[2])
                elif props:
                    pass          # elements after the vertex table are not needed
            elif tok[0] == "property" and in_vertex:
                if tok[1] == "list":
                    raise ValueError("list properties in the vertex element are not supported")
                props.append((tok[2], _PLY_TYPES[tok[1]]))
            elif tok[0] == "end_header":
                break
        if fmt == "ascii":
            rows = np.loadtxt(f, max_rows=n, ndmin=2)
            return {name: rows[:, i].astype(t) for i, (name, t) in enumerate(props)}
        order = "<" if fmt == "binary_little_endian" else ">"
        dt = np.dtype([(name, order + t) for name, t in props])
        raw = np.frombuffer(f.read(n * dt.itemsize), dtype=dt, count=n)
        return {name: np.ascontiguousarray(raw[name]) for name, _ in props}


def load_ply(path: str, device="cpu") -> Dict[str, torch.Tensor]:
    """{'xyz' [P,3], 'f_dc' [P,C], 'opacity' [P,1], 'scaling' [P,S], 'rotation' [P,4]} as float32 tensors, and 'obj_prob'
    [P,K] when (and only when) the file has ``obj_prob_*`` properties."""
    v = read_vertex_table(path)

    def stack(prefix):
        keys = sorted((k for k in v if k.startswith(prefix)), key=lambda k: int(k.split("_")[-1]))
        return np.stack([v[k] for k in keys], axis=1).astype(np.float32)

    out = {"xyz": np.stack([v["x"], v["y"], v["z"]], axis=1).astype(np.float32), "f_dc": stack("f_dc_"),
           "opacity": v["opacity"].astype(np.float32)[:, None], "scaling": stack("scale_"), "rotation": stack("rot_")}
    if any(k.startswith("obj_prob_") for k in v):
        out["obj_prob"] = stack("obj_prob_")
    return {k: torch.from_numpy(a).to(device) for k, a in out.items()}


# ---- triangle meshes (monogs_amd.tsdf) ------------------------------------------------------------------------------------
def save_mesh_ply(path: str, mesh) -> None:
    """An indexed triangle mesh (``vertices`` [V,3], ``triangles`` [T,3], ``colors`` [V,3] in 0..1 or None) as a binary
    little-endian PLY: ``vertex`` x y z (+ uchar red green blue) and ``face`` with ``list uchar int vertex_indices`` -- the layout
    MeshLab and Open3D read.  An empty mesh writes a valid file with zero elements."""
    v = mesh.vertices.detach().to("cpu", torch.float32).numpy().reshape(-1, 3)
    f = mesh.triangles.detach().to("cpu", torch.int32).numpy().reshape(-1, 3)
    col = None if mesh.colors is None else mesh.colors.detach().to("cpu", torch.float32).numpy().reshape(-1, 3)
    vdt = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")] + ([("red", "u1"), ("green", "u1"), ("blue", "u1")] if col is not None else [])
    vt = np.zeros(v.shape[0], dtype=vdt)
    vt["x"], vt["y"], vt["z"] = v[:, 0], v[:, 1], v[:, 2]
    if col is not None:
        u8 = np.floor(np.clip(col, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
        vt["red"], vt["green"], vt["blue"] = u8[:, 0], u8[:, 1], u8[:, 2]
    ft = np.zeros(f.shape[0], dtype=[("n", "u1"), ("i", "<i4", (3,))])
    ft["n"], ft["i"] = 3, f
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % v.shape[0]
    header += "property float x\nproperty float y\nproperty float z\n"
    if col is not None:
        header += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    header += "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % f.shape[0]
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(vt.tobytes())
        fh.write(ft.tobytes())


_PLY_INDEX_TYPES = {"int": "<i4", "int32": "<i4", "uint": "<u4", "uint32": "<u4"}


def _read_faces(path, raw, nf, index_type):
    """int32 [T,3] from the face records ``uchar n, n indices``: all triangles (one strided view), all quads (each split (0,1,2),
    (0,2,3)), or a mix of the two (walked record by record).  Indices beyond 2^31 - 1 are refused."""
    out = None
    for n in (3, 4):
        fdt = np.dtype([("n", "u1"), ("i", index_type, (n,))])
        if len(raw) >= nf * fdt.itemsize:
            ft = np.frombuffer(raw, dtype=fdt, count=nf)
            if (ft["n"] == n).all():
                out = ft["i"].astype(np.int64).reshape(-1, n)
                break
    if out is None:
        rows, at = [], 0
        for _ in range(nf):
            if at >= len(raw):
                raise ValueError(f"{path}: truncated face list")
            n = raw[at]
            if n not in (3, 4) or at + 1 + 4 * n > len(raw):
                raise ValueError(f"{path}: only faces of three or four vertices are read")
            rows.append(np.frombuffer(raw, dtype=index_type, count=n, offset=at + 1).astype(np.int64))
            at += 1 + 4 * n
        out_rows = []
        for r in rows:
            out_rows.append(r[[0, 1, 2]])
            if len(r) == 4:
                out_rows.append(r[[0, 2, 3]])
        out = np.stack(out_rows) if out_rows else np.zeros((0, 3), np.int64)
    elif out.shape[1] == 4:
        out = np.stack([out[:, [0, 1, 2]], out[:, [0, 2, 3]]], axis=1).reshape(-1, 3)
    if out.size and (out.max() > 0x7FFFFFFF or out.min() < 0):
        raise ValueError(f"{path}: vertex index outside int32")
    return np.ascontiguousarray(out.astype(np.int32)).reshape(-1, 3)


def load_mesh_ply(path: str, device="cpu"):
    """The ``TriangleMesh`` of a binary little-endian PLY: a file ``save_mesh_ply`` wrote (colours come back as uchar / 255), or one
    whose faces are ``list uchar int|uint vertex_indices`` of three or four vertices (a quad is split (0,1,2), (0,2,3): how Replica's
    ``mesh.ply`` comes)."""
    from .tsdf import TriangleMesh
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        nv = nf = 0
        props, element, index_type = [], None, "<i4"
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: truncated header")
            tok = line.decode("ascii").split()
            if not tok or tok[0] == "comment":
                continue
            if tok[0] == "format" and tok[1] != "binary_little_endian":
                raise ValueError(f"{path}: only binary_little_endian mesh files are read")
            if tok[0] == "element":
                element = tok[1]
                if element == "vertex":
                    nv = int(tok[2])
                elif element == "face":
                    nf = int(tok[2])
            elif tok[0] == "property" and element == "vertex":
                props.append((tok[2], "<" + _PLY_TYPES[tok[1]]))
            elif tok[0] == "property" and element == "face":
                if (len(tok) != 5 or tok[1] != "list" or tok[2] not in ("uchar", "uint8") or tok[3] not in _PLY_INDEX_TYPES
                        or tok[4] not in ("vertex_indices", "vertex_index")):
                    raise ValueError(f"{path}: face property {tok[1:]} is not 'list uchar int|uint vertex_indices'")
                index_type = _PLY_INDEX_TYPES[tok[3]]
            elif tok[0] == "end_header":
                break
        vdt = np.dtype(props)
        vt = np.frombuffer(f.read(nv * vdt.itemsize), dtype=vdt, count=nv)
        raw = f.read()
    faces = _read_faces(path, raw, nf, index_type)
    v = np.stack([vt["x"], vt["y"], vt["z"]], axis=1).astype(np.float32).reshape(-1, 3)
    col = None
    if "red" in vt.dtype.names:
        col = (np.stack([vt["red"], vt["green"], vt["blue"]], axis=1).astype(np.float32) / 255.0).reshape(-1, 3)
    return TriangleMesh(torch.from_numpy(v).to(device), torch.from_numpy(faces).to(device),
                        None if col is None else torch.from_numpy(col).to(device))
