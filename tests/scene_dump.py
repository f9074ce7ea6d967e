"""A PyrSceneDesc as a flat file, for the probes that pack a scene without a device (tests/probes/pack_check.cpp): the fields in
declaration order, scalars raw, each array as a 64-bit byte count and its bytes -- 0 for NULL."""
import ctypes as C

import numpy as np

from pyrite_amd import abi

# pointer field -> (the field that counts its elements, bytes per element): the one table of how long each array is
ARRAYS = {
    "tri_positions": ("num_triangles", 36), "tri_normals": ("num_triangles", 36), "tri_uvs": ("num_triangles", 24), "tri_material": ("num_triangles", 4),
    "spheres": ("num_spheres", 16), "sphere_tex_scale": ("num_spheres", 8), "sphere_material": ("num_spheres", 4),
    "planes": ("num_planes", 32), "plane_material": ("num_planes", 4),
    "lamps": ("num_lamps", C.sizeof(abi.PyrLamp)), "materials": ("num_materials", C.sizeof(abi.PyrMaterial)), "components": ("num_components", C.sizeof(abi.PyrComponent)),
    "programs": ("num_programs", C.sizeof(abi.PyrProgram)), "instrs": ("num_instrs", C.sizeof(abi.PyrInstr)),
    "spectra": ("num_spectra", C.sizeof(abi.PyrSpectrum)), "spectrum_data": ("num_spectrum_floats", 4), "rgb_basis": ("rgb_basis_count", 12),
    "textures": ("num_textures", C.sizeof(abi.PyrTexture)), "texture_data": ("num_texture_floats", 4),
    "tri_frames": ("num_triangles", 48), "plane_frames": ("num_planes", 16),
}


def dump(desc):
    """The bytes of the dump of `desc` (a PyrSceneDesc whose arrays are alive, as FlatScene.desc() returns it)."""
    out = []
    for name, kind in abi.PyrSceneDesc._fields_:
        value = getattr(desc, name)
        if name not in ARRAYS:
            out.append(bytes(kind(value)))
            continue
        counter, size = ARRAYS[name]
        n = int(getattr(desc, counter)) * size if value else 0
        out.append(np.uint64(n).tobytes())
        if n:
            out.append(C.string_at(C.cast(value, C.c_void_p), n))
    return b"".join(out)


def write(path, desc):
    with open(path, "wb") as f:
        f.write(dump(desc))
