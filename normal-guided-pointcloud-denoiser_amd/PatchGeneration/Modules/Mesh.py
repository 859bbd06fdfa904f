"""Mesh container + normal-guided vertex update (drop-in for PatchGeneration/Modules/Mesh.py, hot-path subset).

`updateVertices(n, k)` (reference Mesh.py:377-418, Vertex_updating.ipynb Algorithm 3) runs k Jacobi sweeps of
    v_i += Σ_{f∋i} Σ_{c∈f} n_f (n_f · (v_c − v_i)) / (3 deg_i)
in fp64 on the HIP device (pcd_mesh_update, one thread per vertex over the vertex->face CSR) and writes the result
back into `self.v` in place, like the reference's `v += scaled_S`.
The vertex-triangle adjacency is igl's format (VF = incident faces grouped by vertex in face order, NI = offsets),
built on the device (pcd_mesh_vta: a stable radix sort of the corners by vertex) and kept there with the faces;
`updateVertices(n, k, fp32=True)` runs the fp32 kernel (pcd_mesh_update_f32).

`denoise(guided_normals=None, ...)` is the reference application's network-free mesh denoiser
(src/GCNDenoiser/GCNDenoiser/MeshNormalFiltering.cpp:170-244): guided bilateral filtering of the face normals over
radius-based face neighbourhoods, vertex_iterations sweeps of the update above after every pass, all on the device
(pcd_mesh_denoise); `getFaceCentroids`, `getFaceAreas`, `getFaceNeighbourhoods` and `filterNormals` are its pieces.
"""
from __future__ import annotations

import numpy as np
import torch

import pcd_native as _nat


def vertex_triangle_adjacency(f: np.ndarray, nv: int):
    """igl.vertex_triangle_adjacency(f, nv) -> (VF, NI)."""
    flat = np.asarray(f, dtype=np.int64).reshape(-1)
    order = np.argsort(flat, kind="stable")
    vf = (order // 3).astype(np.int64)
    counts = np.bincount(flat, minlength=nv)
    ni = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return vf, ni


class Mesh:
    def __init__(self, v, f, noise_factor=0, f2f=None, vta=None, gt=None):
        self._topo = {}           # device copies of the faces and the adjacency, per precision
        self.v = v
        self.f = f
        self.noise_factor = noise_factor
        self.f2f = f2f
        self.vta = vta            # igl (VF, NI); None: built on the device on first use (pcd_mesh_vta)
        self.gt = gt

    # assigning the faces or the adjacency drops the device copies built from them
    @property
    def f(self):
        return self._f

    @f.setter
    def f(self, value):
        self._f = value
        self._topo = {}

    @property
    def vta(self):
        return self._vta

    @vta.setter
    def vta(self, value):
        self._vta = value
        self._topo = {}

    @property
    def f2f(self):
        return self._f2f

    @f2f.setter
    def f2f(self, value):
        self._f2f = value         # igl TT [nf, 3]; None: built on the device on first use (pcd_mesh_tta)
        self._topo = {}

    @classmethod
    def readFile(cls, file_path: str) -> "Mesh":
        from Pointcloud.Modules.Object import read_obj_arrays
        v, _, f, _ = read_obj_arrays(file_path)
        return cls(v, f)

    def getVertices(self):
        return self.v

    def getFaceNormals(self):
        """Unit normals of (v1 − v0) × (v2 − v1) per face (Mesh.py:110-114)."""
        fvs = self.getVertices()[self.f]
        cr = np.cross(fvs[:, 1, :] - fvs[:, 0, :], fvs[:, 2, :] - fvs[:, 1, :])
        return cr / np.linalg.norm(cr, axis=1)[:, None]

    def getVertexTriangleAdjacency(self):
        if self.vta is None:
            vf, ni = self._topology(False)[1:]
            self._vta = (vf.cpu().numpy(), ni.cpu().numpy())   # (the device copies it came from stay valid)
        return self.vta

    def _topology(self, fp32: bool):
        """(faces, VF, NI) on the device, int32 for the fp32 path, int64 for fp64; the adjacency is the caller's vta
        when one was given, else built on the device.  Cached per precision together with a host copy of the faces
        it was built from: an in-place edit of self.f (same object, new contents) rebuilds it."""
        key = bool(fp32)
        hit = self._topo.get(key)
        if hit is not None and not np.array_equal(hit[0], self.f):
            hit = None
        if hit is None:
            it = torch.int32 if fp32 else torch.int64
            f_host = np.array(self.f, copy=True)
            fd = torch.as_tensor(np.ascontiguousarray(f_host)).to(_nat.device()).to(it).contiguous()
            if self.vta is not None:
                vf, ni = (torch.as_tensor(np.ascontiguousarray(a)).to(fd.device).to(it) for a in self.vta)
            else:
                vf, ni = _nat.mesh_vta(fd, len(self.v), out_dtype=it)
            hit = (f_host, fd, vf.contiguous(), ni.contiguous())
            self._topo[key] = hit
        return hit[1:]

    def updateVertices(self, n, k=15, fp32: bool = False):
        """Mesh.py:377-418: k Jacobi sweeps, in place on self.v.  fp32=True runs the fp32 kernel (float4 rows, int32
        topology) instead of the reference's fp64 arithmetic."""
        v = self.getVertices()
        fd, vfd, nid = self._topology(fp32)
        dev = fd.device
        dt = torch.float32 if fp32 else torch.float64
        vd = torch.as_tensor(np.ascontiguousarray(v)).to(dev).to(dt).contiguous()
        nd = torch.as_tensor(np.ascontiguousarray(n)).to(dev).to(dt).contiguous()
        assert nd.shape == fd.shape, "one normal per face"
        if fp32:
            _nat.mesh_update_f32(vd, fd, nd, vfd, nid, k)
        else:
            _nat.mesh_update(vd, fd, nd, vfd, nid, k)
        v[...] = vd.cpu().numpy().astype(v.dtype, copy=False)

    # ------------------------------------------------------------------------------ guided bilateral normal filtering
    # The reference's network-free mesh denoiser (src/GCNDenoiser/GCNDenoiser/MeshNormalFiltering.cpp:170-244) on one
    # device: face geometry, the mean centroid distance of edge-adjacent faces, the face neighbourhoods and the filter
    # pass are HIP kernels (csrc/mesh.hip); the neighbourhoods and the geometry behind them are always fp64.
    def _geometry(self):
        """(v, f, vf, ni, centroid, area, normal) in fp64 / int64 on the device, for the current vertices."""
        fd, vfd, nid = self._topology(False)
        nv = len(self.getVertices())
        if fd.numel() and (int(fd.min()) < 0 or int(fd.max()) >= nv):      # (a caller's vta is not checked elsewhere)
            raise ValueError("Mesh: face index out of range [0, nv)")
        vd = torch.as_tensor(np.ascontiguousarray(self.getVertices())).to(fd.device).to(torch.float64).contiguous()
        return (vd, fd, vfd, nid) + _nat.mesh_face_geometry(vd, fd)

    def getFaceCentroids(self):
        """(p0 + p1 + p2) / 3 per face (MeshDenoisingBase::getFaceCentroid, MeshDenoisingBase.cpp:44-52), fp64."""
        return self._geometry()[4].cpu().numpy()

    def getFaceAreas(self):
        """0.5 |(p1 − p0) × (p1 − p2)| per face (MeshDenoisingBase::getFaceArea, MeshDenoisingBase.cpp:24-42), fp64."""
        return self._geometry()[5].cpu().numpy()

    def getMeanCentroidDistance(self):
        """Mean |c_f − c_g| over the ordered pairs of faces sharing an edge: getRadius / getSigmaS with multiple = 1
        (MeshNormalFiltering.cpp:134-168)."""
        _, fd, vfd, nid, c, _, _ = self._geometry()
        return float(_nat.mesh_face_scale(c, fd, vfd, nid)[0])

    def _neighbourhoods(self, mode, multiple_radius, radius, geometry=None):
        """The CSR (offsets, faces) int64 on the device.  Cached with the topology (assigning f or vta drops it) and
        with a host copy of the vertices it was measured on: radius-based rows depend on the centroids."""
        if mode not in ("radius", "vertex"):
            raise ValueError(f"Mesh: unknown neighbourhood mode {mode!r} (radius, vertex)")
        if mode == "radius":
            if radius is not None and not float(radius) >= 0:
                raise ValueError("Mesh: radius must be >= 0")
            if radius is None and not float(multiple_radius) > 0:
                raise ValueError("Mesh: multiple_radius must be > 0")
        key = ("nbr", mode) + ((None if radius is None else float(radius), float(multiple_radius))
                               if mode == "radius" else ())
        self._topology(False)                                   # (drops the cache when f was edited in place)
        hit = self._topo.get(key)
        if hit is not None and not (np.array_equal(hit[4], self.f) and
                                    (mode != "radius" or np.array_equal(hit[0], self.getVertices()))):
            hit = None
        if hit is None:
            _, fd, vfd, nid, c, _, _ = geometry if geometry is not None else self._geometry()
            nf = fd.size(0)
            if mode == "vertex":                                # bound: the degrees of the three corners
                deg = nid[1:] - nid[:-1]
                cap = deg[fd].sum(1) if nf else torch.zeros(0, dtype=torch.int64, device=fd.device)
                r = 0.0
            else:
                r = float(radius) if radius is not None else \
                    float(multiple_radius) * float(_nat.mesh_face_scale(c, fd, vfd, nid)[0])
                if not np.isfinite(r):
                    raise ValueError("Mesh: the neighbourhood radius is not finite")
                # bound: the Euclidean ball count over the fp32 centroids, the radius widened by their rounding
                if nf:
                    c32 = c.to(torch.float32)
                    r32 = np.nextafter(np.float32((r + 4e-7 * float(c.abs().max())) * (1 + 1e-6)), np.float32(np.inf))
                    cap = _nat.Grid(c32).radius_counts(c32, torch.full((nf,), float(r32), device=c.device))
                else:
                    cap = torch.zeros(0, dtype=torch.int64, device=fd.device)
            off, nbr = _nat.mesh_neighbourhoods(c, fd, vfd, nid, 0 if mode == "radius" else 1, r, cap.contiguous())
            hit = (np.array(self.getVertices(), copy=True) if mode == "radius" else None, off, nbr, {},
                   np.array(self.f, copy=True))
            self._topo[key] = hit
        return hit[1], hit[2], hit[3]

    def getFaceNeighbourhoods(self, mode="radius", multiple_radius=2, radius=None):
        """Face neighbourhoods as a CSR (offsets [nf+1], faces), rows in ascending face index, the face itself
        included.  radius: faces reachable over vertex-sharing steps that stay within `radius` (default
        multiple_radius x the mean centroid distance of edge-adjacent faces) of the centre's centroid
        (MeshNormalFiltering::getRadiusBasedFaceNeighbor, MeshNormalFiltering.cpp:47-78) -- not the Euclidean ball;
        vertex: faces sharing a vertex (MeshDenoisingBase.cpp:75-92)."""
        off, nbr, _ = self._neighbourhoods(mode, multiple_radius, radius)
        return off.cpu().numpy(), nbr.cpu().numpy()

    @staticmethod
    def _check_filter_args(nf, mode, sigma_r, multiple_sigma_s, **normals):
        if mode not in ("radius", "vertex"):
            raise ValueError(f"Mesh: unknown neighbourhood mode {mode!r} (radius, vertex)")
        if not float(sigma_r) > 0 or not float(multiple_sigma_s) > 0:
            raise ValueError("Mesh: sigma_r and multiple_sigma_s must be > 0")
        for name, a in normals.items():
            if a is not None and np.shape(a) != (nf, 3):
                raise ValueError(f"Mesh: {name} must have one normal per face, shape ({nf}, 3), got {np.shape(a)}")

    def filterNormals(self, guided=None, normals=None, sigma_r=0.3, multiple_sigma_s=1, mode="radius",
                      multiple_radius=2, radius=None, fp32: bool = False):
        """One pass of the guided bilateral filter (MeshNormalFiltering.cpp:207-236) over the current mesh; returns the
        filtered unit normals [nf, 3].  guided: the guidance normals (None: the mesh's own face normals); normals: the
        normals being averaged (None: the guidance, as in the reference's first iteration)."""
        nf = len(self.f)
        self._check_filter_args(nf, mode, sigma_r, multiple_sigma_s, guided=guided, normals=normals)
        geo = self._geometry()
        _, fd, vfd, nid, c, area, n = geo
        off, nbr, extra = self._neighbourhoods(mode, multiple_radius, radius, geo)
        scale = _nat.mesh_face_scale(c, fd, vfd, nid)
        dt = torch.float32 if fp32 else torch.float64
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(c.device).to(dt).contiguous()
        g = n.to(dt) if guided is None else dev(guided)
        src = g if normals is None else dev(normals)
        if fp32:
            off, nbr = self._csr32(off, nbr, extra)
        out = _nat.mesh_filter(c.to(dt), area.to(dt), g, src, off, nbr, sigma_r, multiple_sigma_s, scale)
        return out.cpu().numpy()

    @staticmethod
    def _csr32(off, nbr, extra):
        if nbr.numel() >= 2 ** 31:
            raise ValueError("Mesh: the fp32 path needs fewer than 2^31 neighbourhood entries")
        if "i32" not in extra:
            extra["i32"] = (off.to(torch.int32), nbr.to(torch.int32))
        return extra["i32"]

    def denoise(self, guided_normals=None, normal_iterations=12, vertex_iterations=16, sigma_r=0.3, multiple_radius=2,
                multiple_sigma_s=1, mode="radius", fp32: bool = False):
        """MeshNormalFiltering::updateFilteredNormalsWithPredictedNormal (MeshNormalFiltering.cpp:170-244, defaults
        :29-40): normal_iterations x {filter the face normals under the fixed guidance, vertex_iterations sweeps of
        updateVertices}, in place on self.v; returns the last filtered normals.  guided_normals=None guides with the
        input mesh's own face normals (bilateral normal filtering).  The neighbourhoods and the radius are those of
        the input mesh.  Vertices in no face keep their position.  fp32=True runs the loop in fp32 (float4 rows, int32
        topology); the neighbourhoods stay fp64."""
        v = self.getVertices()
        nf = len(self.f)
        self._check_filter_args(nf, mode, sigma_r, multiple_sigma_s, guided_normals=guided_normals)
        if int(normal_iterations) < 0 or int(vertex_iterations) < 0:
            raise ValueError("Mesh: iteration counts must be >= 0")
        geo = self._geometry()
        off, nbr, extra = self._neighbourhoods(mode, multiple_radius, None, geo)
        dt = torch.float32 if fp32 else torch.float64
        if guided_normals is not None and not isinstance(guided_normals, torch.Tensor):
            guided_normals = np.ascontiguousarray(guided_normals)     # (a device tensor stays on the device)
        g = None if guided_normals is None else torch.as_tensor(guided_normals).to(off.device).to(dt).contiguous()
        if int(normal_iterations) == 0 or nf == 0:
            return (geo[6].to(dt) if g is None else g).cpu().numpy()
        fd, vfd, nid = self._topology(fp32)
        if fp32:
            off, nbr = self._csr32(off, nbr, extra)
        vd = geo[0].to(dt).contiguous()
        out = _nat.mesh_denoise(vd, fd, vfd, nid, off, nbr, g, normal_iterations, vertex_iterations, sigma_r,
                                multiple_sigma_s)
        v[...] = vd.cpu().numpy().astype(v.dtype, copy=False)
        return out.cpu().numpy()

    # ------------------------------------------------------------------------------------- patches (GCN network input)
    # The selection half of the reference's patch pipeline (Mesh.py:141-163, 189-204, 242-251, 300-305) on the device:
    # the edge adjacency (pcd_mesh_tta), the two-ring radius and the face centre (pcd_patch_radius), and the faces with
    # a vertex strictly inside the ball as a CSR (pcd_patch_select_*).  PatchCollector builds the network rows on top.
    def _adjacency(self):
        """igl.triangle_triangle_adjacency(f)[0] as int64 [nf, 3] on the device: the caller's f2f when one was given,
        else built on the device; cached with the topology."""
        fd = self._topology(False)[0]
        hit = self._topo.get("tta")
        if hit is not None and not np.array_equal(hit[0], self.f):     # (f edited in place)
            hit = None
        if hit is None:
            if self.f2f is not None:
                tt = torch.as_tensor(np.ascontiguousarray(self.f2f)).to(fd.device).to(torch.int64).contiguous()
                if tuple(tt.shape) != (fd.size(0), 3):
                    raise ValueError(f"Mesh: f2f must have shape ({fd.size(0)}, 3), got {tuple(tt.shape)}")
            else:
                tt = _nat.mesh_tta(fd, len(self.getVertices()))
            hit = (np.array(self.f, copy=True), tt)
            self._topo["tta"] = hit
        return hit[1]

    def getTriangleTriangleAdjacency(self):
        """igl.triangle_triangle_adjacency(f)[0]: [nf, 3], slot e = the face across the edge (f[e], f[(e+1)%3]), -1 on
        a boundary edge and on an edge shared by more than two faces."""
        if self.f2f is None:
            self._f2f = self._adjacency().cpu().numpy()          # (the device copy it came from stays valid)
        return self.f2f

    def getNeighbourhood(self, face_index, ring):
        """The faces within `ring` edge steps of face_index, ascending (Mesh.py:193-204); absent neighbours are
        skipped, where the reference's -1 adds the last face of the mesh."""
        if ring < 1:
            return np.array([])
        f2f = self.getTriangleTriangleAdjacency()
        result = np.array([face_index], dtype=np.int64).reshape(-1)
        for _ in range(ring):
            nb = f2f[result].reshape(-1)
            result = np.union1d(result, nb[nb >= 0])
        return result

    def getAreas(self, faces):
        """0.5 |(v1 - v0) x (v2 - v0)| of the given faces (Mesh.py:144-150)."""
        t = self.getVertices()[np.asarray(self.f)[np.asarray(faces).astype(int)]]
        return 0.5 * np.linalg.norm(np.cross(t[..., 1, :] - t[..., 0, :], t[..., 2, :] - t[..., 0, :], axis=-1), axis=-1)

    def _patch_state(self):
        """What every patch query needs, on the device and cached against host copies of the vertices and faces:
        (v fp64, f, vf, ni, tt, the grid over the fp32 vertices, max |coordinate|, the number of zero-area faces)."""
        fd, vfd, nid = self._topology(False)
        tt = self._adjacency()
        hit = self._topo.get("patch")
        if hit is not None and not (np.array_equal(hit[0], self.getVertices()) and np.array_equal(hit[1], self.f)):
            hit = None
        if hit is None:
            vd, _, _, _, _, area, _ = self._geometry()
            if not bool(torch.isfinite(vd).all()):
                raise ValueError("Mesh: the vertices are not finite")
            grid = _nat.Grid(vd.to(torch.float32)) if vd.size(0) else None
            hit = (np.array(self.getVertices(), copy=True), np.array(self.f, copy=True), vd, grid,
                   float(vd.abs().max()) if vd.numel() else 0.0, int((~(area > 0)).sum()))
            self._topo["patch"] = hit
        return (hit[2], fd, vfd, nid, tt) + hit[3:]

    def _faces_arg(self, fis):
        """The requested faces as int64 on the device, every one checked against [0, nf)."""
        nf = len(self.f)
        a = np.arange(nf, dtype=np.int64) if fis is None else np.asarray(fis)
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise ValueError("Mesh: face indices must be integers")
        a = a.astype(np.int64).reshape(-1)
        if a.size and (a.min() < 0 or a.max() >= nf):
            raise ValueError(f"Mesh: face index out of range [0, {nf})")
        return torch.as_tensor(a).to(_nat.device())

    def _patch_balls(self, fis_d, k):
        """(centre [n,3], r [n]) fp64 on the device for the faces fis_d (int64, on the device, in range)."""
        vd, fd, _, _, tt = self._patch_state()[:5]
        return _nat.patch_radius(vd, fd, tt, fis_d, k)

    def _patches(self, fis_d, k, out=None, state=None):
        """(centre, r, offsets, faces) of the patches of fis_d on the device.  The candidates of the exact fp64 test are
        the rows of the grid over the fp32 vertices in the cells around the ball, each radius widened by the rounding of
        the coordinates (as _neighbourhoods widens its own).  out: the int64
        device buffer to fill instead of one of the exact size (ValueError, nothing written, if it is too small)."""
        vd, fd, vfd, nid, tt, grid, vmax, _ = state if state is not None else self._patch_state()
        centre, r = _nat.patch_radius(vd, fd, tt, fis_d, k)
        n = fis_d.size(0)
        if n == 0 or grid is None:
            z = torch.zeros(n + 1, dtype=torch.int64, device=fd.device)
            return centre, r, z, torch.zeros(0, dtype=torch.int64, device=fd.device)
        if not bool(torch.isfinite(r).all()):
            raise ValueError("Mesh: a patch radius is not finite")
        off, faces = _nat.patch_select(grid, 4e-7 * vmax, vd, fd, vfd, nid, centre, r, out)
        return centre, r, off, faces

    def getPatchRadius(self, fis=None, k=4):
        """r = k sqrt(mean area of the two-ring) per face of fis (Mesh.selectPaperPatch, Mesh.py:301-303), float64."""
        return self._patch_balls(self._faces_arg(fis), k)[1].cpu().numpy()

    def getPatchFaces(self, fis=None, k=4):
        """The patches of the faces fis as a CSR (offsets [n+1], faces), rows ascending: every face with a vertex
        strictly within r of the face's centre, over the whole mesh (Mesh.getFacesInRange, Mesh.py:157-163)."""
        _, _, off, faces = self._patches(self._faces_arg(fis), k)
        return off.cpu().numpy(), faces.cpu().numpy()
