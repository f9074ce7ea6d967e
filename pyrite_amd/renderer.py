"""Host-side mirror of the reference's renderer seam.

    Renderer::render(&self, film, task_runner, on_status, camera, world, resources)   pyrite/src/renderer/mod.rs:77-111

`World` is the frozen scene (World::from_project + Resources), `Camera` the perspective camera
(cameras.rs:20-27), `Renderer` the parameter block (renderer/mod.rs:18-28). `Renderer.render` hands the call to
libpyrite_gpu.so -- the HIP kernels are the only implementation; nothing here computes radiance on the CPU."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi
from ._lib import check, lib
from .compiler import FlatScene, camera_from_project, renderer_from_project
from .film import Film


def weld(positions, normals):
    """Corner labels for `World.set_smoothing` from a mesh's own arrays: `positions` and `normals` are [n,3,3] or [n,9] float32,
    and two corners get the same label exactly when all six words -- the bits of position and normal -- agree. Returns uint32
    [n,3]; a label is the index of the first corner of its group. A mesh whose rest normals break along an edge keeps that
    crease, since the corners on its two sides differ in their normals."""
    p = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
    n = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
    if p.shape != n.shape or len(p) % 3:
        raise ValueError("weld needs positions and normals of one shape [n,3,3], not %r and %r" % (np.shape(positions), np.shape(normals)))
    if len(p) == 0:
        return np.zeros((0, 3), dtype=np.uint32)
    words = np.concatenate([p, n], axis=1).view(np.uint32)
    _, first, inverse = np.unique(words, axis=0, return_index=True, return_inverse=True)
    return first[inverse.reshape(-1)].astype(np.uint32).reshape(-1, 3)


class World:
    """World::from_project (world.rs:39-271) result. Device scenes are created lazily, one per device."""

    def __init__(self, flat: FlatScene):
        self.flat = flat
        self._desc = flat.desc()
        self._scenes = {}
        self._builders = {}
        self._objects = [dict(o) for o in flat.objects]  # what moves together (World.pose)
        self._poses = {}  # object index -> (float32[16] column-major, scale): the poses the scenes are in; identity where absent
        self._skins = {}  # object index -> dict(joints uint16 [T,3,4], weights float32 [T,3,4], num_joints): the bindings (World.set_skins)
        self._joints = {}  # object index -> float32 [J,16] column-major: the joints the scenes are in; identity where absent
        self._morphs = {}  # object index -> dict(positions float32 [T,n,3,3], normals float32 [T,n,3,3] | None): the targets (World.set_morphs)
        self._weights = {}  # object index -> float32 [T]: the weights the scenes are in; zero where absent
        self._smoothing = {}  # object index -> uint32 [n,3]: the corner labels (World.set_smoothing)
        self._smooth_frame = False  # a pose, skin or morph has run since the smoothing was set: the scenes hold recomputed normals

    @classmethod
    def from_project(cls, world, base_dir="."):
        return cls(FlatScene().add_world(world, base_dir))

    @property
    def desc(self):
        return self._desc

    BUILDERS = {"host": abi.PYR_BUILD_HOST, "device": abi.PYR_BUILD_DEVICE}

    def scene(self, device=0, slot=0, build=None):
        """The PyrScene on `device` (`slot` > 0: a further copy on the same device, for the one-GPU multi-rank test rig).
        `build`: who builds the acceleration structure when the scene is created here, "host" (one CPU thread; the default) or
        "device" (pyr_scene_create_with: the same rules on the GPU and, where no node needs the median fallback, the same tree).
        A scene that exists already is returned as it was built; asking for another builder then is an error."""
        if build is not None and build not in self.BUILDERS:
            raise ValueError("build must be 'host' or 'device', not %r" % (build,))
        key = device if slot == 0 else (device, slot)
        if key not in self._scenes:
            handle = C.c_void_p()
            if build is None:
                check(lib().pyr_scene_create(C.byref(self._desc), int(device), C.byref(handle)))
            else:
                params = abi.PyrBuildParams(builder=self.BUILDERS[build])
                check(lib().pyr_scene_create_with(C.byref(self._desc), int(device), C.byref(params), C.byref(handle)))
            self._scenes[key] = handle
            self._builders[key] = build or "host"
            if self._objects:  # the rest pose is the description; a scene made after a pose is built for the pose it is in
                self._set_objects(handle)
                if self._skins:
                    self._set_skins(handle, self._skins)
                if self._morphs:
                    self._set_morphs(handle, self._morphs)
                if self._smoothing:
                    self._set_smoothing(handle, self._smoothing)
                if any(np.any(w != 0) for w in self._weights.values()):
                    self._send(handle, "morph", self._poses, self._joints if self._skins else None, self._weights, "rebuild", 0)
                elif self._joints:
                    self._send(handle, "skin", self._poses, self._joints, None, "rebuild", 0)
                elif self._poses or self._smooth_frame:  # (a smoothed object's normals are recomputed under the identity too)
                    self._send(handle, "pose", self._poses, None, None, "rebuild", 0)
        elif build is not None and build != self._builders[key]:
            raise ValueError("the scene on device %r was created with build=%r" % (device, self._builders[key]))
        return self._scenes[key]

    def build_info(self, device=0, slot=0):
        """pyr_scene_build_info as a dict: the builder asked for and used, why they differ, levels, median splits, the tree's
        digest and the stage times of scene creation in milliseconds."""
        info = abi.PyrBuildInfo()
        check(lib().pyr_scene_build_info(self.scene(device, slot), C.byref(info)))
        return {name: getattr(info, name) for name, _ in info._fields_ if name != "reserved"}

    def bvh_info(self, device=0):
        info = abi.PyrBvhInfo()
        check(lib().pyr_scene_bvh_info(self.scene(device), C.byref(info)))
        return {name: int(getattr(info, name)) for name, _ in info._fields_}

    UPDATE_MODES = {"refit": abi.PYR_UPDATE_REFIT, "rebuild": abi.PYR_UPDATE_REBUILD}
    IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1], dtype=np.float32)

    @property
    def objects(self):
        """What moves together: one record per project object that has geometry (a sphere; a mesh) and per add_triangles call,
        or what set_objects named -- `name`, `first_triangle`, `num_triangles`, `first_sphere`, `num_spheres`."""
        return [dict(o) for o in self._objects]

    def _set_objects(self, handle, objects=None):
        objects = self._objects if objects is None else objects
        ranges = (abi.PyrObjectRange * max(1, len(objects)))()
        for k, o in enumerate(objects):
            ranges[k] = abi.PyrObjectRange(o.get("first_triangle", 0), o.get("num_triangles", 0), o.get("first_sphere", 0), o.get("num_spheres", 0))
        check(lib().pyr_scene_set_objects(handle, ranges, len(objects)))

    def set_objects(self, objects=None):
        """Names other primitive ranges as the objects (pyr_scene_set_objects on every scene of this world; None: the records of
        the description again). The geometry as it is now becomes the rest pose, and every pose is the identity again."""
        if (self._poses or self._joints or self._weights or self._smooth_frame) and self._scenes:  # every scene of this world is in the same pose: `flat` follows the first
            self._follow(self._geometry(next(iter(self._scenes.values()))))
        objects = [dict(o) for o in (self.flat.objects if objects is None else objects)]
        for handle in self._scenes.values():
            self._set_objects(handle, objects)
        self._objects = objects
        self._forget()  # skins, morphs and the smoothing hang on objects: pyr_scene_set_objects forgot them

    def _forget(self):
        """Every pose is the identity again, and what hangs on objects is gone."""
        self._poses, self._skins, self._joints, self._morphs, self._weights = {}, {}, {}, {}, {}
        self._smoothing, self._smooth_frame = {}, False

    def _follow(self, arrays):
        for name, attr in (("positions", "tri_positions"), ("normals", "tri_normals"), ("frames", "tri_frames"), ("spheres", "spheres")):
            if arrays.get(name) is not None and len(arrays[name]):
                setattr(self.flat, attr, [np.array(arrays[name], dtype=np.float32).reshape(len(arrays[name]), -1)])
        self._desc = self.flat.desc()

    def _pose_records(self, poses):
        records = (abi.PyrObjectPose * max(1, len(self._objects)))()
        for k in range(len(self._objects)):
            matrix, scale = poses.get(k, (None, 1.0))
            m = self.IDENTITY if matrix is None else np.asarray(matrix, dtype=np.float32)
            if m.shape == (4, 4):
                m = m.T  # rows of a 4x4 array -> column-major
            m = np.ascontiguousarray(m, dtype=np.float32).reshape(-1)
            if m.size != 16:
                raise ValueError("the pose of object %d is not a 4x4 matrix" % k)
            records[k].transform = (C.c_float * 16)(*[float(x) for x in m])
            records[k].scale = float(scale)
        return records

    def _send(self, handle, entry, poses, tables, weights, mode, stream):
        """pyr_scene_<entry> on one scene with the widest update that entry has: the poses; for "skin" and "morph" the joint table
        (`tables` None: the scene keeps its joints); for "morph" the weight table."""
        common = dict(mode=self.UPDATE_MODES[mode], num_objects=len(self._objects), poses=self._pose_records(poses))
        u = {"pose": abi.PyrPoseUpdate, "skin": abi.PyrSkinUpdate, "morph": abi.PyrMorphUpdate}[entry](**common)
        if tables is not None:
            joints = [tables[index] if index in tables else np.tile(self.IDENTITY, (self._skins[index]["num_joints"], 1)) for index in sorted(self._skins)]
            joints = np.ascontiguousarray(np.concatenate(joints) if joints else np.zeros((0, 16)), dtype=np.float32)
            u.joints, u.num_joints = joints.ctypes.data, len(joints)
        if entry == "morph":
            rows = [weights[index] if index in weights else np.zeros(len(self._morphs[index]["positions"]), dtype=np.float32) for index in sorted(self._morphs)]
            table = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros(0), dtype=np.float32)
            u.weights, u.num_weights = table.ctypes.data, len(table)
        check(getattr(lib(), "pyr_scene_" + entry)(handle, C.byref(u), C.c_void_p(int(stream))))

    def _frame(self, entry, poses, joints, weights, mode, device, stream):
        """One frame through pyr_scene_<entry>: checks what was given, merges it with what the world is in (None keeps), sends it to
        the scene on `device` and remembers the result for scenes created later."""
        if mode not in self.UPDATE_MODES:
            raise ValueError("mode must be 'refit' or 'rebuild', not %r" % (mode,))
        for k in ({} if poses is None else poses):
            if not 0 <= int(k) < len(self._objects):
                raise ValueError("no object %r: the world has %d" % (k, len(self._objects)))
        merged = dict(self._weights)
        if entry == "morph":
            for index, w in weights.items():
                if int(index) not in self._morphs:
                    raise ValueError("no morph on object %r" % (index,))
                w = np.ascontiguousarray(w, dtype=np.float32)
                if w.shape != (len(self._morphs[int(index)]["positions"]),):
                    raise ValueError("the morph of object %r has %d targets, not %r weights" % (index, len(self._morphs[int(index)]["positions"]), w.shape))
                merged[int(index)] = w
            if not self._morphs:
                raise ValueError("the world has no morphs (set_morphs gives them)")
            if joints is not None and not self._skins:
                raise ValueError("joints are given, and the world has no skins")
        tables = None if joints is None else self._joint_tables(joints)
        named = self._poses if poses is None else {int(k): (None if v[0] is None else np.array(v[0], dtype=np.float32), float(v[1])) for k, v in poses.items()}
        self._send(self.scene(device), entry, named, tables, merged, mode, stream)
        self._poses, self._weights = named, merged
        if tables is not None:
            self._joints = tables
        self._smooth_frame = bool(self._smoothing)

    def pose(self, poses, mode="refit", device=0, stream=0):
        """Poses the objects of the scene on `device` (pyr_scene_pose): `poses` maps an object's index in `World.objects` to
        (matrix, scale) -- a 4x4 array as written on paper (translation in the last column), or 16 floats column-major, or None
        for no transform; the uniform scale comes first. Objects it does not name keep the identity: every pose is from the
        rest pose, never from the previous one. The primitives are computed on the GPU; mode as for `update`. `World.flat`
        stays the rest pose, and the world remembers the poses for scenes it creates later."""
        self._frame("pose", poses, None, None, mode, device, stream)

    def keep_previous(self, keep=True, device=0):
        """Keeps the geometry of the scene on `device` as it is now as the previous frame's (pyr_scene_keep_previous): the
        motion pass finds each hit's material point there, whatever update, pose or skin follows. Call it after a frame is
        done and before the scene moves on; `keep=False` drops the snapshot."""
        check(lib().pyr_scene_keep_previous(self.scene(device), 1 if keep else 0))

    def _set_skins(self, handle, skins):
        order = sorted(skins)
        records = (abi.PyrSkin * max(1, len(order)))()
        for k, index in enumerate(order):
            s = skins[index]
            records[k] = abi.PyrSkin(object=index, num_joints=s["num_joints"], joints=s["joints"].ctypes.data, weights=s["weights"].ctypes.data)
        check(lib().pyr_scene_set_skins(handle, records, len(order)))
        if any(skins[index]["blend"] != "linear" for index in order):  # (pyr_scene_set_skins has made every skin linear)
            modes = (C.c_uint32 * len(order))(*[self.SKIN_BLENDS[skins[index]["blend"]] for index in order])
            check(lib().pyr_scene_set_skin_blend(handle, modes, len(order)))

    SKIN_BLENDS = {"linear": abi.PYR_SKIN_LINEAR, "dual_quaternion": abi.PYR_SKIN_DUAL_QUATERNION}

    def set_skins(self, skins):
        """Binds meshes to joints (pyr_scene_set_skins on every scene of this world): `skins` maps an object's index in
        `World.objects` to dict(joints=uint16 [T,3,4], weights=float32 [T,3,4], num_joints=J) for that object's T triangles --
        four joint indices below J and four weights per vertex -- and, if wanted, blend="linear" (the default: the vertex's
        matrix is the weighted sum of its joints' matrices) or "dual_quaternion" (pyr_scene_set_skin_blend: the joints are blended
        as rigid motions, which keeps the volume of a twisting mesh; the joints of such a skin must be rotations and
        translations). Skins are in the order of their object indices. Every joint is the identity afterwards and the geometry
        does not change; an empty dict forgets the skins."""
        bound = {}
        for index, s in skins.items():
            if not 0 <= int(index) < len(self._objects):
                raise ValueError("no object %r: the world has %d" % (index, len(self._objects)))
            shape = (self._objects[int(index)].get("num_triangles", 0), 3, 4)
            joints, weights = np.asarray(s["joints"]), np.asarray(s["weights"])
            if joints.shape != shape or weights.shape != shape:
                raise ValueError("the skin of object %r needs joints and weights of shape %r, not %r and %r" % (index, shape, joints.shape, weights.shape))
            if joints.size and (joints.min() < 0 or joints.max() > 0xFFFF):
                raise ValueError("the skin of object %r names a joint index that is no uint16" % (index,))
            blend = s.get("blend", "linear")
            if blend not in self.SKIN_BLENDS:
                raise ValueError("the skin of object %r has blend %r: it must be 'linear' or 'dual_quaternion'" % (index, blend))
            bound[int(index)] = dict(joints=np.ascontiguousarray(joints, dtype=np.uint16), weights=np.ascontiguousarray(weights, dtype=np.float32), num_joints=int(s["num_joints"]),
                                     blend=blend)
        for handle in self._scenes.values():
            self._set_skins(handle, bound)
        self._skins, self._joints = bound, {}

    def _joint_tables(self, joints):
        """{object: float32 [J,16] column-major} of `joints`, checked against the skins."""
        tables = {}
        for index, table in joints.items():
            if int(index) not in self._skins:
                raise ValueError("no skin on object %r" % (index,))
            t = np.asarray(table, dtype=np.float32)
            if t.ndim == 3 and t.shape[1:] == (4, 4):
                t = t.transpose(0, 2, 1)  # rows of a 4x4 array -> column-major
            t = np.ascontiguousarray(t, dtype=np.float32).reshape(len(t), -1)
            if t.shape != (self._skins[int(index)]["num_joints"], 16):
                raise ValueError("the joints of object %r are not %d 4x4 matrices" % (index, self._skins[int(index)]["num_joints"]))
            tables[int(index)] = t
        return tables

    def skin(self, joints, poses=None, mode="refit", device=0, stream=0):
        """One frame of the skinned meshes of the scene on `device` (pyr_scene_skin): `joints` maps a skinned object's index to its
        joint matrices, [J,4,4] as written on paper or [J,16] column-major; a skin it does not name is at the identity. Every
        vertex takes the matrix blended from its four joints by its weights, then the object's pose: `poses` as for `pose`, None
        keeps the poses the world is in. Everything is computed from the rest pose on the GPU; mode as for `update`. `World.flat`
        stays the rest pose, and the world remembers joints and poses for scenes it creates later."""
        self._frame("skin", poses, joints, None, mode, device, stream)

    def _set_morphs(self, handle, morphs):
        order = sorted(morphs)
        records = (abi.PyrMorph * max(1, len(order)))()
        for k, index in enumerate(order):
            m = morphs[index]
            records[k] = abi.PyrMorph(object=index, num_targets=len(m["positions"]), position_deltas=m["positions"].ctypes.data,
                                      normal_deltas=None if m["normals"] is None else m["normals"].ctypes.data)
        check(lib().pyr_scene_set_morphs(handle, records, len(order)))

    def set_morphs(self, morphs):
        """Gives meshes their morph targets (pyr_scene_set_morphs on every scene of this world): `morphs` maps an object's index in
        `World.objects` to dict(positions=float32 [T,n,3,3], normals=None | float32 [T,n,3,3]) for T targets (1 to 256) over that
        object's n triangles -- position deltas and, if the normals are to follow, normal deltas. Morphs are in the order of their
        object indices. Every weight is zero afterwards and the geometry does not change; an empty dict forgets the morphs."""
        held = {}
        for index, m in morphs.items():
            if not 0 <= int(index) < len(self._objects):
                raise ValueError("no object %r: the world has %d" % (index, len(self._objects)))
            positions = np.asarray(m["positions"])
            normals = None if m.get("normals") is None else np.asarray(m["normals"])
            n = self._objects[int(index)].get("num_triangles", 0)
            if positions.ndim != 4 or positions.shape[1:] != (n, 3, 3) or not 1 <= positions.shape[0] <= 256:
                raise ValueError("the morph of object %r needs positions of shape [1..256, %d, 3, 3], not %r" % (index, n, positions.shape))
            if normals is not None and normals.shape != positions.shape:
                raise ValueError("the morph of object %r needs normals of shape %r, not %r" % (index, positions.shape, normals.shape))
            held[int(index)] = dict(positions=np.ascontiguousarray(positions, dtype=np.float32), normals=None if normals is None else np.ascontiguousarray(normals, dtype=np.float32))
        for handle in self._scenes.values():
            self._set_morphs(handle, held)
        self._morphs, self._weights = held, {}

    def morph(self, weights, joints=None, poses=None, mode="refit", device=0, stream=0):
        """One frame of the morphed meshes of the scene on `device` (pyr_scene_morph): `weights` maps a morphed object's index to
        one weight per target, [T]; a morph it does not name stays at the weights it is in. Every vertex takes the weighted deltas
        of the targets whose weight is not zero, then its skin if the object has one -- `joints` as for `skin`, None keeps the
        joints the world is in -- then the object's pose: `poses` as for `pose`, None keeps the poses. Everything is computed from
        the rest pose on the GPU; mode as for `update`. `World.flat` stays the rest pose, and the world remembers weights, joints
        and poses for scenes it creates later."""
        self._frame("morph", poses, joints, weights, mode, device, stream)

    def _set_smoothing(self, handle, smoothing):
        order = sorted(smoothing)
        records = (abi.PyrSmoothing * max(1, len(order)))()
        for k, index in enumerate(order):
            records[k] = abi.PyrSmoothing(object=index, vertex_ids=smoothing[index].ctypes.data)
        check(lib().pyr_scene_set_smoothing(handle, records, len(order)))

    def _rest_of(self, index):
        """(positions [n,9], normals [n,9]) of an object's triangles in the rest pose, which `World.flat` stays."""
        o = self._objects[index]
        t0, n = o.get("first_triangle", 0), o.get("num_triangles", 0)
        cat = lambda rows: np.concatenate([np.asarray(r, dtype=np.float32).reshape(-1, 9) for r in rows]) if len(rows) else np.zeros((0, 9), dtype=np.float32)  # noqa: E731
        return cat(self.flat.tri_positions)[t0:t0 + n], cat(self.flat.tri_normals)[t0:t0 + n]

    def set_smoothing(self, smoothing):
        """Has the normals of meshes recomputed from where their surface is (pyr_scene_set_smoothing on every scene of this
        world): `smoothing` maps an object's index in `World.objects` to one label per corner of that object's n triangles,
        integers [n,3] -- corners with equal labels share a vertex normal, the area-weighted sum of their triangles' face
        vectors -- or to None: `weld` of the object's rest positions and rest normals, which keeps the creases the rest normals
        already have. From then on every `pose`, `skin` and `morph` recomputes those objects' normals and tangent frames on the
        GPU from the positions of the frame, also under the identity. The geometry does not change at this call; an empty dict
        forgets the smoothing, and so do `set_objects` and an `update` that carries arrays."""
        held = {}
        for index, ids in smoothing.items():
            if not 0 <= int(index) < len(self._objects):
                raise ValueError("no object %r: the world has %d" % (index, len(self._objects)))
            n = self._objects[int(index)].get("num_triangles", 0)
            if n == 0:
                raise ValueError("object %r has no triangles to smooth" % (index,))
            if ids is None:
                ids = weld(*self._rest_of(int(index)))
            ids = np.asarray(ids)
            if ids.shape != (n, 3) or ids.dtype.kind not in "iu" or (ids.size and (ids.min() < 0 or ids.max() > 0xFFFFFFFF)):
                raise ValueError("the smoothing of object %r needs uint32 labels of shape (%d, 3), not %s %r" % (index, n, ids.dtype, ids.shape))
            held[int(index)] = np.ascontiguousarray(ids, dtype=np.uint32)
        for handle in self._scenes.values():
            self._set_smoothing(handle, held)
        self._smoothing = held
        if not held:
            self._smooth_frame = False

    def geometry(self, device=0):
        """The geometry of the scene on `device` as it is now (pyr_scene_geometry): a dict of float32 arrays `positions` [n,9],
        `normals` [n,9], `frames` [n,12] (None unless the scene keeps frames) and `spheres` [n,4]."""
        return self._geometry(self.scene(device))

    def _geometry(self, handle):
        nt, ns = self._desc.num_triangles, self._desc.num_spheres
        out = {"positions": np.zeros((nt, 9), dtype=np.float32), "normals": np.zeros((nt, 9), dtype=np.float32),
               "frames": np.zeros((nt, 12), dtype=np.float32) if self.flat.uses_normal_maps and nt else None, "spheres": np.zeros((ns, 4), dtype=np.float32)}
        pointer = lambda a: None if a is None or a.size == 0 else a.ctypes.data  # noqa: E731
        check(lib().pyr_scene_geometry(handle, pointer(out["positions"]), pointer(out["normals"]), pointer(out["frames"]), pointer(out["spheres"])))
        return out

    def update(self, positions=None, normals=None, frames=None, spheres=None, mode="refit", device=0, stream=0):
        """Moves the geometry of the scene on `device` (pyr_scene_update): new `positions` [n,3,3], `normals` [n,3,3], `frames`
        [n,3,4] for the same triangles and `spheres` [n,4] for the same spheres; what is None stays. mode="refit" keeps the
        tree's topology and recomputes every box; "rebuild" builds a new tree with the scene's builder. Arrays that are torch
        tensors on the GPU go through pyr_scene_update_device on `stream` (all of them must be, then); anything else is taken
        as host data. `World.flat` and the description follow, so a scene created later elsewhere is the moved one. New arrays are
        a new geometry, not a pose of the old one: the scene forgets its objects, and `set_objects()` names them again."""
        if mode not in self.UPDATE_MODES:
            raise ValueError("mode must be 'refit' or 'rebuild', not %r" % (mode,))
        given = {"positions": (positions, 9), "normals": (normals, 9), "frames": (frames, 12), "spheres": (spheres, 4)}
        on_device = [a is not None and hasattr(a, "data_ptr") and getattr(a, "is_cuda", False) for a, _ in given.values()]
        some = [a is not None for a, _ in given.values()]
        if any(on_device) and on_device != some:
            raise ValueError("the arrays of one update are all host arrays or all device tensors")
        u = abi.PyrGeometryUpdate(mode=self.UPDATE_MODES[mode], num_triangles=self._desc.num_triangles, num_spheres=self._desc.num_spheres)
        host, keep = {}, []
        for name, (a, width) in given.items():
            if a is None:
                continue
            count = self._desc.num_spheres if name == "spheres" else self._desc.num_triangles
            if any(on_device):
                import torch

                t = a.to(torch.float32).contiguous()
                if t.numel() != count * width:
                    raise ValueError("%s holds %d floats, the scene needs %d" % (name, t.numel(), count * width))
                keep.append(t)
                host[name] = t.detach().cpu().numpy().reshape(count, width)
                pointer = t.data_ptr()
            else:
                h = np.ascontiguousarray(a, dtype=np.float32)
                if h.size != count * width:
                    raise ValueError("%s holds %d floats, the scene needs %d" % (name, h.size, count * width))
                host[name] = h.reshape(count, width)
                pointer = host[name].ctypes.data
            if name == "frames" and not self.flat.uses_normal_maps:
                continue  # the description passes frames only for normal maps (FlatScene.desc): the device keeps none to move
            setattr(u, {"positions": "tri_positions", "normals": "tri_normals", "frames": "tri_frames", "spheres": "spheres"}[name], pointer)
        if any(on_device):
            check(lib().pyr_scene_update_device(self.scene(device), C.byref(u), C.c_void_p(int(stream))))
        else:
            check(lib().pyr_scene_update(self.scene(device), C.byref(u)))
        del keep
        if u.tri_positions or u.tri_normals or u.tri_frames or u.spheres:
            self._forget()  # new arrays are a new geometry, not a pose of the old one: the scene forgot its objects (set_objects names them again)
        for name, attr in (("positions", "tri_positions"), ("normals", "tri_normals"), ("frames", "tri_frames"), ("spheres", "spheres")):
            if name in host:
                setattr(self.flat, attr, [host[name].copy()])
        self._desc = self.flat.desc()

    def update_info(self, device=0):
        """pyr_scene_update_info as a dict: the last update's mode, schedule length, updates since the last build, stage times in
        milliseconds, and area_ratio -- the binary tree's summed child box areas now over those at the last build."""
        info = abi.PyrUpdateInfo()
        check(lib().pyr_scene_update_info(self.scene(device), C.byref(info)))
        return {name: getattr(info, name) for name, _ in info._fields_ if name != "reserved"}

    def intersect(self, rays, device=0, want_counters=False):
        """World::intersect (world.rs:273-299) for float32 rays [n,6] -> (structured hits, kernel ms, counters|None)."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        hits = np.zeros(len(rays), dtype=np.dtype([("distance", "<f4"), ("shape", "<u4"), ("u", "<f4"), ("v", "<f4")]))
        ms = C.c_float(0)
        counters = abi.PyrCounters()
        check(lib().pyr_scene_intersect(self.scene(device), rays.ctypes.data, len(rays), hits.ctypes.data, C.byref(ms),
                                        C.byref(counters) if want_counters else None))
        return hits, float(ms.value), (counters.as_dict() if want_counters else None)

    def close(self):
        for handle in self._scenes.values():
            lib().pyr_scene_destroy(handle)
        self._scenes = {}
        self._builders = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Camera:
    def __init__(self, pyr_camera: abi.PyrCamera):
        self.c = pyr_camera

    @classmethod
    def from_project(cls, cam):
        return cls(camera_from_project(cam))


class Renderer:
    """Renderer (renderer/mod.rs:18-28) for Algorithm::Simple. `seed` has no reference counterpart (the reference
    seeds from OS entropy, simple.rs:26-28)."""

    def __init__(self, pixel_samples, bounces=8, light_samples=4, spectrum_samples=10, spectrum_bins=64, spectrum_span=(380.0, 780.0),
                 tile_size=32, seed=1):
        self.pixel_samples, self.bounces, self.light_samples = int(pixel_samples), int(bounces), int(light_samples)
        self.spectrum_samples, self.spectrum_bins, self.spectrum_span = int(spectrum_samples), int(spectrum_bins), tuple(spectrum_span)
        self.tile_size, self.seed = int(tile_size), int(seed)

    @classmethod
    def from_project(cls, r, seed=1):
        return cls(seed=seed, **renderer_from_project(r))

    def new_film(self, width, height):  # main.rs:190-195
        return Film(width, height, self.spectrum_bins, self.spectrum_span)

    def num_tiles(self, width, height):  # make_tiles, renderer/algorithm.rs:158-166
        ts = self.tile_size
        return ((width + ts - 1) // ts) * ((height + ts - 1) // ts)

    def params(self, flags=0, tile_range=None, film_rows=None, share=None, sample_begin=0):
        """PyrRenderParams of this renderer. `tile_range` / `film_rows` restrict the call to raster tiles [a, b) and to a window of
        pixel rows; `share` (pyrite_amd.distributed.Share) sets tiles, stride and film layout at once; `sample_begin` makes the call
        render the samples [sample_begin, sample_begin + pixel_samples) of every pixel's budget."""
        p = abi.PyrRenderParams()
        p.bounces, p.pixel_samples, p.light_samples = self.bounces, self.pixel_samples, self.light_samples
        p.spectrum_samples, p.tile_size, p.flags, p.seed = self.spectrum_samples, self.tile_size, flags, self.seed
        if tile_range is not None:
            p.tile_begin, p.tile_end = int(tile_range[0]), int(tile_range[1])
        if film_rows is not None:
            p.film_row_begin, p.film_row_count = int(film_rows[0]), int(film_rows[1])
        if share is not None:
            share.apply(p)
        p.sample_begin = int(sample_begin)
        return p

    def session(self, film_size, camera: Camera, world: World, halves=False, device=0, film: Film = None):
        """A progressive render of this renderer's whole budget (pyr_session_*): `film_size` = (width, height). The film lives on
        the GPU; with `film` the session continues from that host Film. See Session."""
        return Session(self, film_size, camera, world, halves=halves, device=device, film=film)

    def features(self, film_size, camera: Camera, world: World, grid=1, albedo_bins=16, device=0):
        """The first-hit feature images of `film_size` = (width, height) (pyr_render_features): albedo film, shading normal,
        depth, coverage, shape and material id per pixel, from grid x grid sub-samples, without noise. See features.Features."""
        from .features import Features

        out = Features(film_size[0], film_size[1], albedo_bins, self.spectrum_span)
        desc, fp = out.albedo.desc(), abi.PyrFeatureParams(int(grid), int(albedo_bins))
        check(lib().pyr_render_features(world.scene(device), C.byref(camera.c), C.byref(desc), C.byref(fp), out.albedo.grains.ctypes.data, out.records.ctypes.data))
        return out

    def motion(self, film_size, camera: Camera, world: World, previous_camera: Camera = None, device=0):
        """The motion records of `film_size` = (width, height) (pyr_render_motion), motion.RECORD [height, width]: per pixel, where
        the surface point `camera` sees was for `previous_camera` (None: the same camera) in the geometry World.keep_previous
        kept -- or in the geometry as it is when none was kept -- its depth there, this frame's depth and shape, and flags."""
        from .motion import RECORD

        out = np.zeros((int(film_size[1]), int(film_size[0])), dtype=RECORD)
        desc = abi.PyrFilmDesc(int(film_size[0]), int(film_size[1]), self.spectrum_bins, self.spectrum_span[0], self.spectrum_span[1] - self.spectrum_span[0])
        previous = camera if previous_camera is None else previous_camera
        check(lib().pyr_render_motion(world.scene(device), C.byref(camera.c), C.byref(previous.c), C.byref(desc), out.ctypes.data))
        return out

    def path_info(self, world: World, device=0):
        """Which kernel a render of `world` with this renderer would run (pyr_scene_path_info): a dict of PyrPathInfo's fields."""
        info, params = abi.PyrPathInfo(), self.params()
        check(lib().pyr_scene_path_info(world.scene(device), C.byref(params), C.byref(info)))
        return {name: int(getattr(info, name)) for name, _ in info._fields_ if name != "reserved"}

    def program_info(self, world: World, device=0):
        """The register files of `world`'s programs (pyr_scene_program_info): largest declared and allocated counts, and whether the
        scene runs the wide interpreter build. A dict of PyrProgramInfo's fields."""
        info = abi.PyrProgramInfo()
        check(lib().pyr_scene_program_info(world.scene(device), C.byref(info)))
        return {name: int(getattr(info, name)) for name, _ in info._fields_ if name != "reserved"}

    def render(self, film: Film, camera: Camera, world: World, on_status=None, device=0, counters=False, tile_range=None, film_rows=None,
               window=None, share=None, sample_begin=0):
        """Blocking render into a host Film (adds to it). Returns the PyrCounters dict when counters=True.
        `tile_range` restricts the call to raster tiles [a, b); with film_rows=(first_row, rows) the exposures go to `window`,
        a float32 [rows, width, bins, 2] array covering only those rows of the image `film` describes."""
        params = self.params(abi.PYR_FLAG_COUNTERS if counters else 0, tile_range, film_rows, share, sample_begin)
        desc = film.desc()
        if window is not None:
            assert window.flags["C_CONTIGUOUS"] and window.dtype == np.float32
            if share is not None:
                assert window.size == share.pixels(film.width) * film.bins * 2
            else:
                assert window.shape == (film_rows[1], film.width, film.bins, 2)
            check(lib().pyr_render_simple(world.scene(device), C.byref(camera.c), C.byref(desc), C.byref(params), window.ctypes.data,
                                          C.cast(None, abi.PyrProgressFn), None))
            return self.counters(world, device) if counters else None
        if on_status is not None:
            cb = abi.PyrProgressFn(lambda user, percent, message: on_status(int(percent), message.decode()))
        else:
            cb = C.cast(None, abi.PyrProgressFn)
        grains = np.ascontiguousarray(film.grains)
        check(lib().pyr_render_simple(world.scene(device), C.byref(camera.c), C.byref(desc), C.byref(params), grains.ctypes.data, cb, None))
        if grains is not film.grains:
            film.grains[...] = grains
        if counters:
            out = abi.PyrCounters()
            check(lib().pyr_scene_counters(world.scene(device), C.byref(out)))
            return out.as_dict()
        return None

    def render_device(self, film_ptr, film_desc, camera: Camera, world: World, stream=0, device=0, flags=0, tile_range=None,
                      film_rows=None, share=None):
        """Asynchronous render into DEVICE memory (`film_ptr` = data_ptr of a float32 tensor laid out as the parameters say:
        [rows, w, bins, 2] pixel rows, or -- with a `share` of tile blocks -- [tiles, ts + 2, ts + 2, bins, 2])."""
        params = self.params(flags, tile_range, film_rows, share)
        check(lib().pyr_render_simple_device(world.scene(device), C.byref(camera.c), C.byref(film_desc), C.byref(params),
                                             C.c_void_p(film_ptr), C.c_void_p(stream)))

    def render_multi(self, film: Film, camera: Camera, world: World, devices, on_status=None):
        """pyr_render_simple_multi: one process driving `devices` (a list of device indices; a repeated index is the one-GPU
        test rig). Blocking; adds into the host Film."""
        handles = (C.c_void_p * len(devices))(*[world.scene(d, slot=i) for i, d in enumerate(devices)])
        params = self.params()
        desc = film.desc()
        cb = abi.PyrProgressFn(lambda user, percent, message: on_status(int(percent), message.decode())) if on_status else C.cast(None, abi.PyrProgressFn)
        grains = np.ascontiguousarray(film.grains)
        check(lib().pyr_render_simple_multi(handles, len(devices), C.byref(camera.c), C.byref(desc), C.byref(params), grains.ctypes.data, cb, None))
        if grains is not film.grains:
            film.grains[...] = grains

    def counters(self, world: World, device=0):
        out = abi.PyrCounters()
        check(lib().pyr_scene_counters(world.scene(device), C.byref(out)))
        return out.as_dict()


class Session:
    """A render cut into passes over the whole image (include/pyrite_gpu.h "progressive sessions"): `render(n)` enqueues the next
    n samples of every pixel and returns at once, `preview()` develops the live film on the GPU and fetches the 8-bit image alone,
    `film()` fetches the film, `noise()` the per-tile noise estimate of a session with `halves`. The world's scene on that device
    serves this session alone until it is closed or synced."""

    def __init__(self, renderer: Renderer, film_size, camera: Camera, world: World, halves=False, device=0, film: Film = None):
        self.renderer, self.world, self.device, self.halves = renderer, world, int(device), bool(halves)
        self.width, self.height = int(film_size[0]), int(film_size[1])
        self._film = renderer.new_film(self.width, self.height) if film is None else film
        assert (self._film.width, self._film.height) == (self.width, self.height)
        self._shape = (self.height, self.width, self._film.bins, 2)
        desc, params = self._film.desc(), renderer.params()
        start = None
        if film is not None:
            start = np.ascontiguousarray(film.grains)
        self.handle = C.c_void_p()
        check(lib().pyr_session_create(world.scene(self.device), C.byref(camera.c), C.byref(desc), C.byref(params),
                                       abi.PYR_SESSION_HALVES if halves else 0, start.ctypes.data if start is not None else None, C.byref(self.handle)))

    @property
    def samples_done(self):
        n = C.c_uint32(0)
        check(lib().pyr_session_samples_done(self.handle, C.byref(n)))
        return int(n.value)

    @property
    def tiles(self):
        """(tiles_x, tiles_y) of the make_tiles grid: the shape of noise()."""
        ts = self.renderer.tile_size
        return (self.width + ts - 1) // ts, (self.height + ts - 1) // ts

    def render(self, samples):
        check(lib().pyr_session_render(self.handle, int(samples)))

    def sync(self):
        check(lib().pyr_session_sync(self.handle))

    def preview(self, step=30.0, filter=None, white=None, tone=None, stats=None):
        """uint8 [height, width, 3]: the film as it stands, developed on the GPU (main.rs:270 uses step 30 for previews). With `tone`
        (develop.tone_params) the film is developed to linear light, measured and tone mapped there (pyr_session_preview_tone) and
        `stats`, an abi.PyrImageStats, is filled when given; without it this is pyr_session_preview's hard clamp."""
        from .develop import develop_params

        p, keep = develop_params(self._film, step, filter, white)
        out = np.zeros((self.height, self.width, 3), dtype=np.uint8)
        if tone is None:
            assert stats is None, "the statistics belong to a tone mapped preview"
            check(lib().pyr_session_preview(self.handle, C.byref(p), out.ctypes.data))
        else:
            check(lib().pyr_session_preview_tone(self.handle, C.byref(p), C.byref(tone), out.ctypes.data, C.byref(stats) if stats is not None else None))
        del keep
        return out

    def linear(self, step=2.0, space="srgb", filter=None, white=None):
        """float32 [height, width, 3]: the film as it stands (A + B with halves) developed to CIE XYZ or linear sRGB on the GPU
        (pyr_session_linear; develop.develop_linear of film() gives the same floats)."""
        from .develop import SPACES, develop_params

        p, keep = develop_params(self._film, step, filter, white)
        out = np.zeros((self.height, self.width, 3), dtype=np.float32)
        check(lib().pyr_session_linear(self.handle, C.byref(p), SPACES[space], out.ctypes.data))
        del keep
        return out

    def film(self):
        """The film so far as a host Film (the sum of the halves when there are two)."""
        out = Film(self.width, self.height, self._film.bins, (self._film.wavelength_start, self._film.wavelength_start + self._film.wavelength_width))
        check(lib().pyr_session_film(self.handle, out.grains.ctypes.data))
        return out

    def features(self, grid=1, albedo_bins=16):
        """Renderer.features for the session's camera and image size, on the session's stream after the passes enqueued so far
        (pyr_session_features). The session's film is not touched."""
        from .features import Features

        out = Features(self.width, self.height, albedo_bins, (self._film.wavelength_start, self._film.wavelength_start + self._film.wavelength_width))
        fp = abi.PyrFeatureParams(int(grid), int(albedo_bins))
        check(lib().pyr_session_features(self.handle, C.byref(fp), out.albedo.grains.ctypes.data, out.records.ctypes.data))
        return out

    def motion(self, previous_camera: Camera):
        """Renderer.motion for the session's camera and image size against `previous_camera`, on the session's stream after the
        passes enqueued so far (pyr_session_motion). The session's film is not touched."""
        from .motion import RECORD

        out = np.zeros((self.height, self.width), dtype=RECORD)
        check(lib().pyr_session_motion(self.handle, C.byref(previous_camera.c), out.ctypes.data))
        return out

    def motion_blurred(self, previous_camera: Camera, step=2.0, filter=None, white=None, **params):
        """float32 [height, width, 3]: the film as it stands developed to linear sRGB and blurred along the motion records against
        `previous_camera`, all on the session's device (pyr_session_motion_blurred; develop.motion_blur of linear() and
        motion(previous_camera) gives the same floats). `params`: develop.motion_blur_params. The session's film is not touched."""
        from .develop import develop_params, motion_blur_params

        p, keep = develop_params(self._film, step, filter, white)
        bp = motion_blur_params(**params)
        out = np.zeros((self.height, self.width, 3), dtype=np.float32)
        check(lib().pyr_session_motion_blurred(self.handle, C.byref(previous_camera.c), C.byref(p), C.byref(bp), out.ctypes.data))
        del keep
        return out

    def lens_blurred(self, step=2.0, filter=None, white=None, grid=1, **params):
        """float32 [height, width, 3]: the film as it stands developed to linear sRGB and blurred by a thin lens over the records of
        the feature pass (`grid` x `grid` sub-samples), all on the session's device (pyr_session_lens_blurred; develop.lens_blur of
        linear() and features(grid).records gives the same floats). `params`: develop.lens_blur_params -- the lens is theirs, not
        the session camera's, which is meant to have rendered with aperture 0. The session's film is not touched."""
        from .develop import develop_params, lens_blur_params

        p, keep = develop_params(self._film, step, filter, white)
        fp, bp = abi.PyrFeatureParams(int(grid), 1), lens_blur_params(**params)
        out = np.zeros((self.height, self.width, 3), dtype=np.float32)
        check(lib().pyr_session_lens_blurred(self.handle, C.byref(p), C.byref(fp), C.byref(bp), out.ctypes.data))
        del keep
        return out

    def glared(self, step=2.0, filter=None, white=None, **params):
        """float32 [height, width, 3]: the film as it stands developed to linear sRGB with the glare added, all on the session's
        device (pyr_session_glared; develop.glare of linear() gives the same floats). `params`: develop.glare_params. The session's
        film is not touched."""
        from .develop import develop_params, glare_params

        p, keep = develop_params(self._film, step, filter, white)
        gp = glare_params(**params)
        out = np.zeros((self.height, self.width, 3), dtype=np.float32)
        check(lib().pyr_session_glared(self.handle, C.byref(p), C.byref(gp), out.ctypes.data))
        del keep
        return out

    def half_films(self):
        """The two half films of a session with `halves`, float32 [height, width, bins, 2] each."""
        a, b = np.zeros(self._shape, dtype=np.float32), np.zeros(self._shape, dtype=np.float32)
        check(lib().pyr_session_halves(self.handle, a.ctypes.data, b.ctypes.data))
        return a, b

    def noise(self):
        """float32 [tiles_y, tiles_x]: relative RMS difference of the half films per tile; half of it estimates the relative
        error of the film (pyr_session_noise). Needs `halves` and two passes."""
        tx, ty = self.tiles
        out = np.zeros((ty, tx), dtype=np.float32)
        check(lib().pyr_session_noise(self.handle, out.ctypes.data))
        return out

    def denoised(self, step=2.0, filter=None, white=None, guides=True, grid=1, albedo_bins=16, **params):
        """(image, error), float32 [height, width, 3] each: the two half films developed to linear sRGB and cross filtered on the
        session's device (pyr_session_denoised; develop.denoise of the developed half_films() gives the same floats). With `guides`
        the feature pass (features(grid, albedo_bins)) runs first and its albedo, normals and depths steer the filter. `params`:
        develop.denoise_params. Needs `halves` and two passes, best an even number of equal ones. The films are not touched."""
        from .develop import denoise_params, develop_params

        p, keep = develop_params(self._film, step, filter, white)
        dp = denoise_params(**params)
        fp = abi.PyrFeatureParams(int(grid), int(albedo_bins)) if guides else None
        out, error = np.zeros((self.height, self.width, 3), dtype=np.float32), np.zeros((self.height, self.width, 3), dtype=np.float32)
        check(lib().pyr_session_denoised(self.handle, C.byref(p), C.byref(fp) if fp is not None else None, C.byref(dp), out.ctypes.data, error.ctypes.data))
        del keep
        return out, error

    def upsampled(self, scale, step=2.0, filter=None, white=None, guides=True, grid=1, albedo_bins=16, denoise=None, **params):
        """float32 [scale*height, scale*width, 3]: the film as it stands, the low image, developed to linear sRGB -- with `denoise`
        (a dict of develop.denoise_params keywords, {} for the defaults) what denoised() gives instead -- and upsampled `scale` times
        under the guidance of the feature pass at both sizes, all on the session's device (pyr_session_upsampled; develop.upsample of
        linear() or denoised() and the two feature passes gives the same floats). Without `guides` no feature pass runs: the plain
        tent. `params`: develop.upsample_params. The session's films are not touched."""
        from .develop import denoise_params, develop_params, upsample_params

        p, keep = develop_params(self._film, step, filter, white)
        up = upsample_params(**params)
        dp = denoise_params(**denoise) if denoise is not None else None
        fp = abi.PyrFeatureParams(int(grid), int(albedo_bins)) if guides else None
        sized = min(max(int(scale), 1), abi.PYR_UPSAMPLE_MOST_SCALE)  # a scale the library refuses never writes
        out = np.zeros((self.height * sized, self.width * sized, 3), dtype=np.float32)
        check(lib().pyr_session_upsampled(self.handle, int(scale), C.byref(p), C.byref(fp) if fp is not None else None, C.byref(dp) if dp is not None else None,
                                          C.byref(up), out.ctypes.data))
        del keep
        return out

    def despeckled(self, step=2.0, filter=None, white=None, denoise=None, guides=True, grid=1, albedo_bins=16, **params):
        """(image, error, removed, counts): the two half films developed to linear sRGB, their fireflies clamped, and then -- with
        `denoise`, a dict of develop.denoise_params keywords, {} for the defaults -- cross filtered as denoised() filters the raw
        halves (`guides`, `grid`, `albedo_bins`: its feature pass), or without it their mean and half their difference, all on the
        session's device (pyr_session_despeckled; develop.despeckle of the developed half_films(), then develop.denoise or the
        mean, gives the same floats). `removed`, `counts`: as develop.despeckle. `params`: develop.despeckle_params. Needs `halves`
        and two passes. The films are not touched."""
        from .develop import denoise_params, despeckle_params, develop_params

        p, keep = develop_params(self._film, step, filter, white)
        sp = despeckle_params(**params)
        dp = denoise_params(**denoise) if denoise is not None else None
        fp = abi.PyrFeatureParams(int(grid), int(albedo_bins)) if guides and dp is not None else None
        out, error, removed = (np.zeros((self.height, self.width, 3), dtype=np.float32) for _ in range(3))
        counts = np.zeros(2, dtype=np.uint32)
        check(lib().pyr_session_despeckled(self.handle, C.byref(p), C.byref(sp), C.byref(fp) if fp is not None else None, C.byref(dp) if dp is not None else None,
                                           out.ctypes.data, error.ctypes.data, removed.ctypes.data, counts.ctypes.data))
        del keep
        return out, error, removed, (int(counts[0]), int(counts[1]))

    def close(self):
        if self.handle:
            lib().pyr_session_destroy(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
