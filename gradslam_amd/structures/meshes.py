"""Meshes: a ragged batch of triangle meshes -- vertices with optional normals and colours, and faces that index them.

The container `TSDFVolume.extract_mesh` returns; it works on CPU tensors too (nothing here calls a kernel).  The geometry
(face normals, areas, surface area, enclosed volume) is plain torch and differentiable w.r.t. the vertices; `save_ply` writes
the file other tools open.  The reference ships no mesh type.
"""
from typing import List, Optional

import numpy as np
import torch

from .pointclouds import Pointclouds

__all__ = ["Meshes"]

_VATTRS = ("verts", "normals", "colors")


class Meshes(object):
    r"""B meshes.  `verts`: a list of (V_b, 3) float tensors; `faces`: a list of (F_b, 3) integer tensors whose entries index the
    rows of verts[b]; `normals`, `colors` (optional): lists shaped like verts, one row per vertex.  Colours are 0..255 as the
    frames hold them.

    Views: `*_list` (per mesh, views of the padded form) and `*_padded` ((B, max V_b, 3) with zero rows, faces (B, max F_b, 3)
    int32 with -1 rows).  Triangles are taken to run counter-clockwise seen from outside."""

    def __init__(self, verts: List[torch.Tensor], faces: List[torch.Tensor], normals: Optional[List[torch.Tensor]] = None,
                 colors: Optional[List[torch.Tensor]] = None):
        if not isinstance(verts, list) or not isinstance(faces, list) or len(verts) == 0:
            raise TypeError("Meshes: verts and faces should be non-empty lists of tensors; got {} and {}".format(type(verts), type(faces)))
        if len(faces) != len(verts):
            raise ValueError("Meshes: verts and faces should have the same length. Got {} and {}.".format(len(verts), len(faces)))
        for name, val in (("normals", normals), ("colors", colors)):
            if val is not None and (not isinstance(val, list) or [tuple(x.shape) for x in val] != [tuple(v.shape) for v in verts]):
                raise ValueError("Meshes: {} should be a list of tensors shaped like verts.".format(name))
        if any(not torch.is_tensor(v) or v.ndim != 2 or v.shape[1] != 3 or not v.is_floating_point() for v in verts):
            raise ValueError("Meshes: every verts tensor should be floating point of shape (V, 3).")
        if any(not torch.is_tensor(f) or f.ndim != 2 or f.shape[1] != 3 or f.is_floating_point() or f.dtype == torch.bool for f in faces):
            raise ValueError("Meshes: every faces tensor should be an integer tensor of shape (F, 3).")
        dev = verts[0].device
        nv, nf = [int(v.shape[0]) for v in verts], [int(f.shape[0]) for f in faces]
        for b, f in enumerate(faces):
            if f.numel() and (int(f.min()) < 0 or int(f.max()) >= nv[b]):
                raise ValueError("Meshes: faces[{}] should index the {} rows of verts[{}]. Got {} .. {}.".format(
                    b, nv[b], b, int(f.min()), int(f.max())))
        pad = lambda xs: None if xs is None else _pad_rows([x.to(dev) for x in xs], max(nv), 0)
        self._adopt(pad(verts), _pad_rows([f.to(dev, torch.int32) for f in faces], max(nf), -1), pad(normals), pad(colors), nv, nf)

    # ------------------------------------------------------------------ bookkeeping
    @classmethod
    def _from_padded(cls, verts, faces, normals, colors, num_verts: List[int], num_faces: List[int]):
        """Adopt padded tensors as they are (padding already in place: zero rows, faces -1): no copy, no check."""
        out = object.__new__(cls)
        out._adopt(verts, faces, normals, colors, num_verts, num_faces)
        return out

    def _adopt(self, verts, faces, normals, colors, num_verts, num_faces):
        self._verts_padded, self._faces_padded, self._normals_padded, self._colors_padded = verts, faces, normals, colors
        self._nv, self._nf = [int(n) for n in num_verts], [int(n) for n in num_faces]
        self.device = verts.device

    def __len__(self):
        return int(self._verts_padded.shape[0])

    has_normals = property(lambda self: self._normals_padded is not None)
    has_colors = property(lambda self: self._colors_padded is not None)
    verts_padded = property(lambda self: self._verts_padded)
    faces_padded = property(lambda self: self._faces_padded)
    normals_padded = property(lambda self: self._normals_padded)
    colors_padded = property(lambda self: self._colors_padded)

    def _list(self, x, counts):
        return None if x is None else [x[b, : counts[b]] for b in range(len(self))]

    verts_list = property(lambda self: self._list(self._verts_padded, self._nv))
    faces_list = property(lambda self: self._list(self._faces_padded, self._nf))
    normals_list = property(lambda self: self._list(self._normals_padded, self._nv))
    colors_list = property(lambda self: self._list(self._colors_padded, self._nv))

    @property
    def num_verts_per_mesh(self):
        return torch.tensor(self._nv, device=self.device)

    @property
    def num_faces_per_mesh(self):
        return torch.tensor(self._nf, device=self.device)

    # ------------------------------------------------------------------ copies
    def _map(self, fn, fn_faces=None):
        opt = lambda x: None if x is None else fn(x)
        return Meshes._from_padded(fn(self._verts_padded), (fn_faces or fn)(self._faces_padded), opt(self._normals_padded),
                                   opt(self._colors_padded), self._nv, self._nf)

    def to(self, device, copy: bool = False):
        if not copy and torch.Tensor().to(device).device == self.device:
            return self
        return self._map(lambda x: x.to(device, copy=copy))

    def cpu(self):
        return self.to(torch.device("cpu"))

    def detach(self):
        return self._map(lambda x: x.detach())

    def clone(self):
        return self._map(lambda x: x.clone())

    def pointclouds(self) -> Pointclouds:
        """The vertices (with their normals and colours) as a Pointclouds that shares storage and gradients with this mesh."""
        out = Pointclouds(device=self.device)
        out._B = len(self)
        out._adopt_padded(self._verts_padded, self._normals_padded, self._colors_padded, None)
        out._set_counts(self._nv)
        return out

    # ------------------------------------------------------------------ geometry (plain torch, differentiable w.r.t. verts)
    def _index(self, index):
        if not isinstance(index, int) or isinstance(index, bool):
            raise TypeError("Index should be int, but was {}.".format(type(index)))
        if not -len(self) <= index < len(self):
            raise IndexError("Meshes: index {} out of range for {} meshes.".format(index, len(self)))
        return index % len(self)

    def face_vertices(self, index: int = 0) -> torch.Tensor:
        """(F, 3, 3): the three corners of every face of mesh `index`."""
        b = self._index(index)
        return self._verts_padded[b][self._faces_padded[b, : self._nf[b]].long()]

    def _face_cross(self, index):
        fv = self.face_vertices(index)
        return torch.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0], dim=-1)

    def face_areas(self, index: int = 0) -> torch.Tensor:
        """(F,): half the length of (v1 - v0) x (v2 - v0); a zero-area face has area 0 and a zero gradient."""
        c = self._face_cross(index)
        sq = (c * c).sum(-1)
        ok = sq > 0
        return torch.where(ok, 0.5 * torch.sqrt(torch.where(ok, sq, torch.ones_like(sq))), torch.zeros_like(sq))

    def face_normals(self, index: int = 0) -> torch.Tensor:
        """(F, 3): (v1 - v0) x (v2 - v0) at unit length -- outward for counter-clockwise faces; zero for a zero-area face."""
        c = self._face_cross(index)
        sq = (c * c).sum(-1, keepdim=True)
        ok = sq > 0
        return torch.where(ok, c / torch.sqrt(torch.where(ok, sq, torch.ones_like(sq))), torch.zeros_like(c))

    def surface_area(self) -> torch.Tensor:
        """(B,): the sum of the face areas of every mesh."""
        return torch.stack([self.face_areas(b).sum() for b in range(len(self))])

    def volume(self) -> torch.Tensor:
        """(B,): the signed sum of v0 . (v1 x v2) / 6 -- the enclosed volume of a closed mesh with outward faces (of an open one:
        that of the cone over it from the coordinate origin)."""
        out = []
        for b in range(len(self)):
            fv = self.face_vertices(b)
            out.append((fv[:, 0] * torch.cross(fv[:, 1], fv[:, 2], dim=-1)).sum() / 6.0)
        return torch.stack(out)

    # ------------------------------------------------------------------ output
    def save_ply(self, path, index: int = 0, binary: bool = True):
        """Write mesh `index` as a PLY file: vertices x y z, normals nx ny nz and colours `uchar red green blue` (0..255, rounded
        and clamped) where the mesh has them, faces as `vertex_indices`; little-endian binary, or ascii.  A device-to-host copy."""
        b = self._index(index)
        host = lambda x: x[b, : self._nv[b]].detach().cpu().numpy().astype("<f4")
        cols = [("x", "y", "z")]
        vert = [host(self._verts_padded)]
        if self.has_normals:
            cols.append(("nx", "ny", "nz"))
            vert.append(host(self._normals_padded))
        rgb = None
        if self.has_colors:
            rgb = np.clip(np.rint(host(self._colors_padded).astype(np.float64)), 0, 255).astype(np.uint8)
        faces = self._faces_padded[b, : self._nf[b]].detach().cpu().numpy().astype("<i4")
        nv, nf = self._nv[b], self._nf[b]
        head = ["ply", "format {} 1.0".format("binary_little_endian" if binary else "ascii"), "comment gradslam_amd Meshes",
                "element vertex {}".format(nv)]
        head += ["property float {}".format(n) for group in cols for n in group]
        if rgb is not None:
            head += ["property uchar {}".format(n) for n in ("red", "green", "blue")]
        head += ["element face {}".format(nf), "property list uchar int vertex_indices", "end_header"]
        with open(path, "wb") as f:
            f.write(("\n".join(head) + "\n").encode("ascii"))
            if binary:
                fields = [(n, "<f4") for group in cols for n in group] + ([(n, "u1") for n in ("red", "green", "blue")] if rgb is not None else [])
                rec = np.zeros(nv, dtype=np.dtype(fields))  # packed: no padding between the fields
                flat = np.concatenate(vert, 1) if nv else np.zeros((0, 3 * len(cols)), "<f4")
                for k, n in enumerate(n for group in cols for n in group):
                    rec[n] = flat[:, k]
                if rgb is not None:
                    for k, n in enumerate(("red", "green", "blue")):
                        rec[n] = rgb[:, k]
                f.write(rec.tobytes())
                frec = np.zeros(nf, dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
                frec["n"] = 3
                frec["v"] = faces
                f.write(frec.tobytes())
            else:
                flat = np.concatenate(vert, 1) if nv else np.zeros((0, 3 * len(cols)), "<f4")
                lines = []
                for r in range(nv):
                    row = [repr(float(x)) for x in flat[r]]  # (the shortest text that reads back to the same float64, hence float32)
                    if rgb is not None:
                        row += [str(int(x)) for x in rgb[r]]
                    lines.append(" ".join(row))
                lines += ["3 {} {} {}".format(*(int(x) for x in faces[r])) for r in range(nf)]
                f.write(("\n".join(lines) + ("\n" if lines else "")).encode("ascii"))

    def open3d(self, index: int = 0, include_colors: bool = True, include_normals: bool = True):
        """Mesh `index` as an `open3d.geometry.TriangleMesh` (a device-to-host copy; colours above 1.1 are taken to be 0..255 and
        normalised, as `Pointclouds.open3d` does).  Needs the `open3d` package."""
        import open3d as o3d

        b = self._index(index)
        take = lambda x: x.detach().cpu().numpy()
        mesh = o3d.geometry.TriangleMesh()
        mesh.vertices = o3d.utility.Vector3dVector(take(self.verts_list[b]).astype(np.float64))
        mesh.triangles = o3d.utility.Vector3iVector(take(self.faces_list[b]).astype(np.int32))
        if self.has_colors and include_colors:
            colors = self.colors_list[b]
            if colors.numel() and (colors.max() > 1.1).item():
                colors = colors / 255
            mesh.vertex_colors = o3d.utility.Vector3dVector(take(torch.clamp(colors, min=0.0, max=1.0)).astype(np.float64))
        if self.has_normals and include_normals:
            mesh.vertex_normals = o3d.utility.Vector3dVector(take(self.normals_list[b]).astype(np.float64))
        return mesh


def _pad_rows(xs, n, value):
    """(B, n, 3) from a list of (n_b, 3) tensors, rows past n_b filled with `value`; differentiable w.r.t. the items."""
    out = []
    for x in xs:
        fill = x.new_full((n - x.shape[0], 3), value)
        out.append(torch.cat([x, fill], 0) if fill.shape[0] else x)
    return torch.stack(out)
