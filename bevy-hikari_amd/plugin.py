"""Host-side mirror of the reference's operator interface for the path.

The reference is a Rust Bevy plugin (no Rust toolchain exists in this image, so the host side
above the C ABI is Python; INTEGRATION.md shows the Rust binding).  Names, fields, defaults and
call order follow cryscan/bevy-hikari v0.3.15:

  HikariSettings / Taa / Upscale / HikariUniversalSettings   src/lib.rs:373-513
  graph.NAME + node names                                     src/lib.rs:43-51
  PrepassNode / LightNode / PostProcessNode  .run()           src/prepass.rs:769, src/light.rs:590, src/post_process.rs:1140
  OverlayNode .run() / Engine.present                         src/overlay.rs:311-395
  FrameCounter                                                src/view.rs:75-103
  HikariPlugin                                                src/lib.rs:95-370

All arithmetic of the path runs in libhikari_hip.so; this module only marshals.
"""
import ctypes as C
import dataclasses
import json
import math
import os
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from . import _ffi as F

ASSETS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "assets")

WORKGROUP_SIZE = 8        # lib.rs:53
NOISE_TEXTURE_COUNT = 16  # lib.rs:54


class graph:  # lib.rs:43-51
    NAME = "hikari"

    class node:
        PREPASS = "hikari_prepass"
        LIGHT = "hikari_light"
        POST_PROCESS = "hikari_post_process"
        OVERLAY = "hikari_overlay"


class Taa:  # lib.rs:466-472
    Jasmine = F.TAA_JASMINE
    NONE = F.TAA_NONE


@dataclass(frozen=True)
class Upscale:  # lib.rs:474-513
    kind: int = F.UPSCALE_SMAA_TU4X
    ratio_: float = 2.0
    sharpness_: float = 0.0

    @staticmethod
    def Fsr1(ratio, sharpness):
        return Upscale(F.UPSCALE_FSR1, ratio, sharpness)

    @staticmethod
    def SmaaTu4x(ratio):
        return Upscale(F.UPSCALE_SMAA_TU4X, ratio, 0.0)

    def ratio(self):
        return min(max(self.ratio_, 1.0), 2.0)

    def sharpness(self):
        return self.sharpness_ if self.kind == F.UPSCALE_FSR1 else 0.0


Upscale.SMAA_TU_1_0 = Upscale.SmaaTu4x(1.0)
Upscale.SMAA_TU_2_0 = Upscale.SmaaTu4x(2.0)


@dataclass
class HikariUniversalSettings:  # lib.rs:373-389
    build_mesh_acceleration_structure: bool = True
    build_instance_acceleration_structure: bool = True


@dataclass
class HikariSettings:  # lib.rs:400-455 (field order and defaults)
    direct_validate_interval: int = 3
    emissive_validate_interval: int = 5
    max_temporal_reuse_count: int = 50
    max_spatial_reuse_count: int = 800
    max_reservoir_lifetime: float = 100.0
    solar_angle: float = 0.046
    indirect_bounces: int = 1
    max_indirect_luminance: float = 10.0
    clear_color: tuple = (0.4, 0.4, 0.4, 1.0)
    temporal_reuse: bool = True
    emissive_spatial_reuse: bool = False
    indirect_spatial_reuse: bool = True
    denoise: bool = True
    taa: int = Taa.Jasmine
    upscale: Upscale = Upscale.SMAA_TU_2_0

    def to_c(self):
        s = F.HkSettings()
        s.direct_validate_interval = self.direct_validate_interval
        s.emissive_validate_interval = self.emissive_validate_interval
        s.max_temporal_reuse_count = self.max_temporal_reuse_count
        s.max_spatial_reuse_count = self.max_spatial_reuse_count
        s.max_reservoir_lifetime = self.max_reservoir_lifetime
        s.solar_angle = self.solar_angle
        s.indirect_bounces = self.indirect_bounces
        s.max_indirect_luminance = self.max_indirect_luminance
        s.clear_color[:] = list(self.clear_color)
        s.temporal_reuse = int(self.temporal_reuse)
        s.emissive_spatial_reuse = int(self.emissive_spatial_reuse)
        s.indirect_spatial_reuse = int(self.indirect_spatial_reuse)
        s.denoise = int(self.denoise)
        s.taa = self.taa
        s.upscale_kind = self.upscale.kind
        s.upscale_ratio = self.upscale.ratio_
        s.upscale_sharpness = self.upscale.sharpness_
        return s


# ---------------------------------------------------------------------------------------------
# 4x4 helpers in plain IEEE doubles, column-major flat lists m[c*4+r] (glam conventions).  Written
# with explicit loops in a fixed order so that the C++ host mirror (include/hikari.hpp) produces the
# SAME f32 uniforms - no BLAS/LAPACK whose summation order could differ in the last bit.
# ---------------------------------------------------------------------------------------------
def _mul4(a, b):
    o = [0.0] * 16
    for c in range(4):
        for r in range(4):
            s = 0.0
            for k in range(4):
                s += a[k * 4 + r] * b[c * 4 + k]
            o[c * 4 + r] = s
    return o


def look_at_transform(eye, target, up=(0.0, 1.0, 0.0)):
    """Transform::from_translation(eye).looking_at(target, up) as a column-major camera-to-world matrix."""
    eye, target, up = ([float(x) for x in v] for v in (eye, target, up))

    def norm(v):
        l = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
        return [v[0] / l, v[1] / l, v[2] / l]

    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]

    f = norm([target[0] - eye[0], target[1] - eye[1], target[2] - eye[2]])
    r = norm(cross(f, up))
    u = cross(r, f)
    return [r[0], r[1], r[2], 0.0, u[0], u[1], u[2], 0.0, -f[0], -f[1], -f[2], 0.0, eye[0], eye[1], eye[2], 1.0]


def _f32(m):
    return np.asarray(m, dtype=np.float64).astype(np.float32)


@dataclass
class Camera:
    """Camera3dBundle with bevy's default PerspectiveProjection (fov pi/4, near 0.1, infinite reverse-Z), or -
    with ortho_height - bevy 0.9's OrthographicProjection (ScalingMode::FixedVertical(ortho_height), near 0,
    far 1000, reverse-Z): the `view.projection[3].w == 1.0` branch of light.wgsl:714-727,1040."""
    transform: list  # column-major 4x4 camera-to-world (16 doubles)
    width: int
    height: int
    fov: float = 0.78539816339744830962
    near: float = 0.1
    ortho_height: Optional[float] = None
    ortho_far: float = 1000.0

    def projection(self):  # Mat4::perspective_infinite_reverse_rh / Mat4::orthographic_rh(l, r, b, t, far, near)
        if self.ortho_height is not None:
            half_h = 0.5 * self.ortho_height
            half_w = half_h * float(self.width) / float(self.height)
            rcp_w, rcp_h, r = 1.0 / (2.0 * half_w), 1.0 / (2.0 * half_h), 1.0 / (self.ortho_far - 0.0)
            m = [0.0] * 16
            m[0], m[5], m[10] = 2.0 * rcp_w, 2.0 * rcp_h, r
            m[12], m[13], m[14], m[15] = 0.0, 0.0, r * self.ortho_far, 1.0
            return m
        f = 1.0 / math.tan(0.5 * self.fov)
        aspect = float(self.width) / float(self.height)
        m = [0.0] * 16
        m[0], m[5], m[11], m[14] = f / aspect, f, -1.0, self.near
        return m

    def inverse_projection(self):
        p = self.projection()
        if self.ortho_height is not None:  # diagonal + translation in z
            m = [0.0] * 16
            m[0], m[5], m[10], m[14], m[15] = 1.0 / p[0], 1.0 / p[5], 1.0 / p[10], -p[14] / p[10], 1.0
            return m
        m = [0.0] * 16
        m[0], m[5], m[11], m[14] = 1.0 / p[0], 1.0 / p[5], 1.0 / p[14], -1.0
        return m

    def inverse_view(self):  # rigid inverse: [R^T | -R^T t]
        t = [float(x) for x in np.asarray(self.transform, dtype=np.float64).reshape(-1)]
        m = [0.0] * 16
        for c in range(3):
            for r in range(3):
                m[c * 4 + r] = t[r * 4 + c]
        for r in range(3):
            m[12 + r] = -(t[r * 4 + 0] * t[12] + t[r * 4 + 1] * t[13] + t[r * 4 + 2] * t[14])
        m[15] = 1.0
        return m

    def view_uniform(self):  # bevy_render 0.9.1 ViewUniform
        t = [float(x) for x in np.asarray(self.transform, dtype=np.float64).reshape(-1)]
        proj, inv_view, inv_proj = self.projection(), self.inverse_view(), self.inverse_projection()
        v = F.HkView()
        v.view_proj[:] = _f32(_mul4(proj, inv_view))
        v.inverse_view_proj[:] = _f32(_mul4(t, inv_proj))  # (P * V^-1)^-1 = V * P^-1
        v.view[:] = _f32(t)
        v.inverse_view[:] = _f32(inv_view)
        v.projection[:] = _f32(proj)
        v.inverse_projection[:] = _f32(inv_proj)
        v.world_position[:] = _f32(t[12:15])
        v.viewport[:] = [0.0, 0.0, float(self.width), float(self.height)]
        return v

    def ray_through(self, u, v):
        """(origin, direction): the world-space ray through the point (u, v) of the image - (0, 0) its top left corner, (1, 1) its
        bottom right one, pixel (x, y)'s centre at ((x + 0.5) / width, (y + 0.5) / height) - as float32[3] each, from the camera's
        own inverse matrices: the point of the near plane under (u, v) is inverse_view_proj * (ndc, 1) (reverse-Z).  A perspective
        ray starts at the eye and runs through that point; an orthographic one starts ON the near plane and runs along the view
        direction, as the primary rays of the prepass do.  The direction is normalised, so a hit's distance is in world units.
        Computed in doubles from the float32 uniforms: the prepass's ray to within rounding, not its bits."""
        vu = self.view_uniform()
        ivp = [float(x) for x in vu.inverse_view_proj]
        ndc = (2.0 * float(u) - 1.0, 1.0 - 2.0 * float(v), 1.0, 1.0)
        q = [0.0] * 4
        for r in range(4):      # (explicit loops in a fixed order, like _mul4: include/hikari.hpp forms the same ray bit for bit)
            s = 0.0
            for c in range(4):
                s += ivp[c * 4 + r] * ndc[c]
            q[r] = s
        near = [q[0] / q[3], q[1] / q[3], q[2] / q[3]]
        if self.ortho_height is not None:
            vp = [float(x) for x in vu.view_proj]
            d = [-vp[2], -vp[6], -vp[10]]      # (light.wgsl:714-727: -normalize(view_proj[0].z, view_proj[1].z, view_proj[2].z))
            origin = near
        else:
            origin = [float(x) for x in vu.world_position]
            d = [near[0] - origin[0], near[1] - origin[1], near[2] - origin[2]]
        l = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        d = [d[0] / l, d[1] / l, d[2] / l]
        origin, d = np.asarray(origin, dtype=np.float64), np.asarray(d, dtype=np.float64)
        return origin.astype(np.float32), d.astype(np.float32)

    def rays_through(self, u, v):
        """ray_through for arrays of points: a RAY_DTYPE array (max_distance 3.4e38, nothing excluded), one ray per (u, v) pair.  The same
        formulas evaluated by numpy in doubles - for batches (picking many points, probe grids), not for bit comparisons."""
        vu = self.view_uniform()
        ivp = np.asarray(list(vu.inverse_view_proj), dtype=np.float64).reshape(4, 4).T   # math layout
        u, v = np.asarray(u, dtype=np.float64).reshape(-1), np.asarray(v, dtype=np.float64).reshape(-1)
        q = np.stack([2.0 * u - 1.0, 1.0 - 2.0 * v, np.ones_like(u), np.ones_like(u)], axis=1) @ ivp.T
        near = q[:, :3] / q[:, 3:4]
        if self.ortho_height is not None:
            vp = np.asarray(list(vu.view_proj), dtype=np.float64)
            origin, d = near, np.broadcast_to(-np.array([vp[2], vp[6], vp[10]]), near.shape)
        else:
            origin = np.broadcast_to(np.asarray(list(vu.world_position), dtype=np.float64), near.shape)
            d = near - origin
        return make_rays(origin, d / np.linalg.norm(d, axis=1, keepdims=True))

    def previous_view_uniform(self, previous: Optional["Camera"] = None):
        cam = previous or self
        v = cam.view_uniform()
        p = F.HkPreviousView()
        p.view_proj[:] = list(v.view_proj)
        p.inverse_view_proj[:] = list(v.inverse_view_proj)
        return p


def lights_uniform(directional=None, ambient_color=(1.0, 1.0, 1.0), ambient_brightness=0.05):
    """bevy AmbientLight default (white, 0.05) and an optional DirectionalLight
    dict(color=(r,g,b) linear, illuminance=lux, direction_to_light=(x,y,z)); bevy scales the colour
    by illuminance / 4800 (exposure of the default camera) before upload."""
    l = F.HkLights()
    l.ambient_color[:] = [c * ambient_brightness for c in ambient_color] + [ambient_brightness]
    if directional:
        scale = directional.get("illuminance", 100000.0) / 4800.0  # bevy_pbr 0.9.1 light.rs exposure
        col = [c * scale for c in directional.get("color", (1.0, 1.0, 1.0))]
        l.directional_color[:] = col + [1.0]
        d = np.asarray(directional["direction_to_light"], dtype=np.float64)
        d = d / np.linalg.norm(d)
        l.direction_to_light[:] = d.astype(np.float32)
        l.n_directional_lights = 1
    return l


# ---------------------------------------------------------------------------------------------
# scene description -> builder
# ---------------------------------------------------------------------------------------------
def linear_to_srgb(c):
    c = float(c)
    return 12.92 * c if c <= 0.0031308 else 1.055 * (c ** (1.0 / 2.4)) - 0.055


def standard_material(base_color_linear=(1, 1, 1, 1), emissive_linear=(0, 0, 0), perceptual_roughness=0.5, metallic=0.0,
                      reflectance=0.5, nonlinear=False):
    """StandardMaterial -> GpuStandardMaterial as material.rs:168-199 does it: `Color -> Vec4` goes
    through bevy 0.9's `From<Color> for Vec4` = as_rgba_f32().  bevy_gltf 0.9.1 builds the colours
    with `Color::rgba(factor)`, for which as_rgba_f32() is the identity, so glTF factors reach the
    GPU buffer unchanged (default).  `nonlinear=True` applies the linear->sRGB encoding that the same
    conversion performs for `Color::rgba_linear` inputs.  Either way these values are INPUTS of the
    boundary; the library never converts colours."""
    m = F.HkMaterial()
    enc = linear_to_srgb if nonlinear else float
    bc = list(base_color_linear) + [1.0] * (4 - len(base_color_linear))
    m.base_color[:] = [enc(bc[0]), enc(bc[1]), enc(bc[2]), float(bc[3])]
    em = list(emissive_linear)
    m.emissive[:] = [enc(em[0]), enc(em[1]), enc(em[2]), 1.0]
    m.base_color_texture = m.emissive_texture = m.metallic_roughness_texture = F.NO_TEXTURE
    m.normal_map_texture = m.occlusion_texture = F.NO_TEXTURE
    m.perceptual_roughness, m.metallic, m.reflectance = perceptual_roughness, metallic, reflectance
    return m


class SceneData:
    """The nine storage buffers of bind group 2 (mesh_material_bindings.wgsl:5-22) as ctypes arrays."""

    FIELDS = ("vertices", "primitives", "asset_nodes", "materials", "instances", "instance_nodes", "emissives", "emissive_nodes",
              "alias_table")

    def __init__(self, previous_transforms=None, **arrays):
        for k in self.FIELDS:
            setattr(self, k, arrays[k])
        #: float32[n_instances][16] or None: PreviousMeshUniform::transform per instance (instance.rs:111-128)
        self.previous_transforms = previous_transforms

    def upload(self, api, ctx):
        n = lambda a: len(a)
        api.call("upload_meshes", ctx, self.vertices, n(self.vertices), self.primitives, n(self.primitives), self.asset_nodes, n(self.asset_nodes))
        api.call("upload_materials", ctx, self.materials, n(self.materials))
        self.upload_instances(api, ctx)

    def upload_instances(self, api, ctx):
        """The instance-level buffers only (what prepare_instances rewrites when something moves)."""
        n = lambda a: len(a)
        api.call("upload_instances", ctx, self.instances, n(self.instances), self.instance_nodes, n(self.instance_nodes), self.emissives,
                 n(self.emissives), self.emissive_nodes, n(self.emissive_nodes), self.alias_table, n(self.alias_table))
        if self.previous_transforms is not None:
            pt = np.ascontiguousarray(self.previous_transforms, dtype=np.float32).reshape(-1, 16)
            assert len(pt) == n(self.instances)
            api.call("upload_previous_transforms", ctx, pt.ctypes.data_as(C.POINTER(F.f32)), len(pt))


class SceneBuilder:
    """hk_scene_builder_*: the Prepare-stage host work (mesh -> BLAS, TLAS, emissives, alias tables)."""

    def __init__(self):
        self.api = F.api()
        self.h = C.c_void_p()
        self.api.call("scene_builder_create", C.byref(self.h))
        self.mesh_vertices = []  # vertex count per mesh id (set_mesh_vertices checks its arrays against it)
        # per instance the id it had when a context last took the instance set, or F.INSTANCE_NEW (Engine.change_instances: the builder
        # shifts ids on removal, so the map is kept here)
        self.origins = []

    def take_origins(self):
        """The origin list of hk_change_scene_instances, consumed: afterwards every instance is its own origin.  Every Engine call that
        hands the builder's instance set to a context consumes it (upload_scene / upload_instances of a SceneData that carries its builder,
        load_scene, update_instances_on_device, change_instances); a host that uploads through raw arrays calls this itself."""
        out = np.array(self.origins, dtype=np.uint32)
        self.origins = list(range(len(self.origins)))
        return out

    def __del__(self):
        if getattr(self, "h", None):
            self.api.raw("scene_builder_destroy")(self.h)
            self.h = None

    def add_mesh(self, positions, normals, uvs, indices=None, topology=F.TOPOLOGY_TRIANGLE_LIST, build_tree=True):
        """hk_scene_builder_add_mesh; build_tree=False: hk_scene_builder_add_mesh_deferred - the mesh gets a stand-in tree of the final
        size and the real one is built by Engine.load_scene (on the device) or build_pending_mesh_trees (on the host)."""
        fn = "scene_builder_add_mesh" if build_tree else "scene_builder_add_mesh_deferred"
        pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        nrm = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        uv = np.ascontiguousarray(uvs, dtype=np.float32).reshape(-1, 2)
        out = F.u32()
        self.mesh_vertices.append(len(pos))
        fp = lambda a: a.ctypes.data_as(C.POINTER(F.f32))
        if indices is None:
            self.api.call(fn, self.h, fp(pos), fp(nrm), fp(uv), len(pos), None, 0, topology, C.byref(out))
        else:
            idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
            self.api.call(fn, self.h, fp(pos), fp(nrm), fp(uv), len(pos), idx.ctypes.data_as(C.POINTER(F.u32)), len(idx), topology, C.byref(out))
        return out.value

    def pending_mesh_trees(self):
        """How many deferred meshes still carry a stand-in tree (hk_scene_builder_pending_mesh_trees)."""
        n = F.u32()
        self.api.call("scene_builder_pending_mesh_trees", self.h, C.byref(n))
        return n.value

    def build_pending_mesh_trees(self):
        """The host completion of the deferred meshes (hk_scene_builder_build_pending_mesh_trees): in place, a finished builder stays
        finished - scene() returns the final arrays."""
        self.api.call("scene_builder_build_pending_mesh_trees", self.h)

    def declare_mesh(self, n_vertices, n_indices=0, topology=F.TOPOLOGY_TRIANGLE_LIST):
        """hk_scene_builder_declare_mesh: a mesh known by its counts, whose arrays are still to come - from device memory
        (Engine.add_meshes(builder, sources=...)) or from the host (resolve_mesh).  n_indices == 0: the identity list over the vertices.
        Until then nothing uploads the builder and no instance may name the mesh."""
        out = F.u32()
        self.api.call("scene_builder_declare_mesh", self.h, int(n_vertices), int(n_indices), topology, C.byref(out))
        self.mesh_vertices.append(int(n_vertices))
        return out.value

    def resolve_mesh(self, mesh_id, positions, normals, uvs=None, indices=None):
        """hk_scene_builder_resolve_mesh: a declared mesh filled from host arrays with add_mesh's arithmetic (uvs None: (0, 0); indices None
        iff it was declared without).  A finished builder stays finished; the mesh then is an ordinary deferred mesh."""
        pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        nrm = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        uv = None if uvs is None else np.ascontiguousarray(uvs, dtype=np.float32).reshape(-1, 2)
        idx = None if indices is None else np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        want = self.mesh_vertices[mesh_id] if mesh_id < len(self.mesh_vertices) else None
        if want is not None and (len(pos) != want or len(nrm) != want or (uv is not None and len(uv) != want)):
            raise ValueError(f"mesh {mesh_id} was declared with {want} vertices")
        fp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(F.f32))
        self.api.call("scene_builder_resolve_mesh", self.h, mesh_id, fp(pos), fp(nrm), fp(uv), None if idx is None else idx.ctypes.data_as(C.POINTER(F.u32)))

    def unresolved_meshes(self):
        """How many declared meshes still wait for their arrays (hk_scene_builder_unresolved_meshes)."""
        n = F.u32()
        self.api.call("scene_builder_unresolved_meshes", self.h, C.byref(n))
        return n.value

    def add_material(self, material):
        out = F.u32()
        self.api.call("scene_builder_add_material", self.h, C.byref(material), C.byref(out))
        return out.value

    def add_instance(self, mesh_id, material_id, transform):
        t = np.ascontiguousarray(transform, dtype=np.float32).reshape(-1)
        out = F.u32()
        self.api.call("scene_builder_add_instance", self.h, mesh_id, material_id, t.ctypes.data_as(C.POINTER(F.f32)), C.byref(out))
        self.origins.append(F.INSTANCE_NEW)
        return out.value

    def set_instance_transform(self, instance_id, transform):
        """Move an instance; the next finish() redoes the instance-level work only."""
        t = np.ascontiguousarray(transform, dtype=np.float32).reshape(-1)
        self.api.call("scene_builder_set_instance_transform", self.h, instance_id, t.ctypes.data_as(C.POINTER(F.f32)))

    def remove_instance(self, instance_id):
        """Take an instance out of the scene (ids of later instances shift down by one)."""
        self.api.call("scene_builder_remove_instance", self.h, instance_id)
        del self.origins[instance_id]

    def set_instance_material(self, instance_id, material_id):
        self.api.call("scene_builder_set_instance_material", self.h, instance_id, material_id)

    def set_material(self, material_id, material):
        """New values for an existing material (hk_scene_builder_set_material): the next finish() redoes the instance-level work only;
        Engine.update_materials(builder) is the device path of the same edit."""
        self.api.call("scene_builder_set_material", self.h, material_id, C.byref(material))

    def set_mesh_vertices(self, mesh_id, positions, normals=None):
        """The host mirror of a deformation (hk_scene_builder_set_mesh_vertices): same topology, tree boxes refit; finish() + upload next."""
        pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1)
        nrm = None if normals is None else np.ascontiguousarray(normals, dtype=np.float32).reshape(-1)
        n = self.mesh_vertices[mesh_id] if 0 <= mesh_id < len(self.mesh_vertices) else None
        if n is None or len(pos) != 3 * n or (nrm is not None and len(nrm) != 3 * n):
            raise ValueError(f"mesh {mesh_id}: expected {n} positions (and normals) of 3 floats")
        self.api.call("scene_builder_set_mesh_vertices", self.h, mesh_id, pos.ctypes.data_as(C.POINTER(F.f32)),
                      None if nrm is None else nrm.ctypes.data_as(C.POINTER(F.f32)))

    def recompute_mesh_normals(self, mesh_id):
        """The host mirror of a device deformation with recompute_normals=True (hk_scene_builder_recompute_mesh_normals): the mesh's normals
        from its current positions, area-weighted, bit for bit what the device stores; after set_mesh_vertices(positions, None)."""
        self.api.call("scene_builder_recompute_mesh_normals", self.h, mesh_id)

    def rebuild_mesh_tree(self, mesh_id):
        """The host mirror of Engine.rebuild_mesh_tree (hk_scene_builder_rebuild_mesh_tree): the mesh's tree built again over its current
        triangles, as add_mesh would build it; finish() + upload next."""
        self.api.call("scene_builder_rebuild_mesh_tree", self.h, mesh_id)

    def mesh_index(self, mesh_id):
        """The HkMeshIndex of a mesh after a finish (what Engine.update_mesh_vertices / skin_mesh take)."""
        out = F.HkMeshIndex()
        self.api.call("scene_builder_mesh_index", self.h, mesh_id, C.byref(out))
        return out

    def mesh_extent(self, mesh_id):
        """The HkMeshExtent of a mesh: its three ranges in the arrays of the LAST finish (node_count 0: no finish has seen it)."""
        out = F.HkMeshExtent()
        self.api.call("scene_builder_mesh_extent", self.h, mesh_id, C.byref(out))
        return out

    def remove_mesh(self, mesh_id):
        """Take a mesh no instance names out of the builder (ids of later meshes shift down by one, the instance declarations follow).
        Returns its HkMeshExtent in the coordinates of the last finish - what Engine.remove_meshes takes, for every removal until the
        next finish() in one call."""
        out = F.HkMeshExtent()
        self.api.call("scene_builder_remove_mesh", self.h, mesh_id, C.byref(out))
        del self.mesh_vertices[mesh_id]   # (the ids behind it shift down: set_mesh_vertices checks its arrays against this list)
        return out

    def finish(self, build_trees=True):
        """hk_scene_builder_finish; build_trees=False: hk_scene_builder_finish_instances (stand-in trees, for a device-side build)."""
        self.api.call("scene_builder_finish" if build_trees else "scene_builder_finish_instances", self.h)
        return self.scene()

    def scene(self):
        """A SceneData from the getters of a finished builder, without finishing it again (after build_pending_mesh_trees or
        Engine.load_scene the arrays of an earlier SceneData are stale by design)."""
        arrays = {}
        for name, typ in (("vertices", F.HkVertex), ("primitives", F.HkPrimitive), ("asset_nodes", F.HkNode), ("materials", F.HkMaterial),
                          ("instances", F.HkInstance), ("instance_nodes", F.HkNode), ("emissives", F.HkEmissive),
                          ("emissive_nodes", F.HkNode), ("alias_table", F.HkAliasEntry)):
            p, n = C.POINTER(typ)(), F.u32()
            self.api.call("scene_builder_" + name, self.h, C.byref(p), C.byref(n))
            arr = (typ * n.value)()
            if n.value:
                C.memmove(arr, p, n.value * C.sizeof(typ))
            arrays[name] = arr
        p, n = C.POINTER(F.f32)(), F.u32()
        self.api.call("scene_builder_previous_transforms", self.h, C.byref(p), C.byref(n))
        prev = np.ctypeslib.as_array(p, shape=(n.value, 16)).copy() if n.value else np.zeros((0, 16), np.float32)
        return SceneData(previous_transforms=prev, **arrays)


def load_cornell(nonlinear_colors=False):
    """examples/cornell.rs:37-41: the glTF scene, flattened by tools/make_fixtures.py."""
    with open(os.path.join(ASSETS, "cornell.json")) as f:
        j = json.load(f)
    b = SceneBuilder()
    mats = []
    for m in j["materials"]:
        # bevy_gltf 0.9.1 load_material: base_color = Color::rgba_linear(factor), emissive = Color::rgb_linear(factor),
        # perceptual_roughness = roughness factor, metallic = metallic factor, reflectance default 0.5
        mats.append(b.add_material(standard_material(m["base_color_factor"], m["emissive_factor"], m["roughness_factor"],
                                                     m["metallic_factor"], 0.5, nonlinear_colors)))
    meshes = [b.add_mesh(m["positions"], m["normals"], m["uvs"], m["indices"]) for m in j["meshes"]]
    for inst in j["instances"]:
        b.add_instance(meshes[inst["mesh"]], mats[j["meshes"][inst["mesh"]]["material"]], inst["transform"])
    scene = b.finish()
    scene.builder = b  # kept for moving instances: builder.set_instance_transform(i, ..) + Engine.refit_instances(builder) / builder.finish()
    return scene


def cornell_camera(width, height):  # examples/cornell.rs:49-50
    return Camera(look_at_transform((0.0, 1.0, 4.0), (0.0, 1.0, 0.0)), width, height)


def load_noise():
    path = os.path.join(ASSETS, "noise_rgba8_16x64x64.bin")
    data = np.fromfile(path, dtype=np.uint8)
    assert data.size == 16 * 64 * 64 * 4
    return data


# ---------------------------------------------------------------------------------------------
# engine: one hk_ctx
# ---------------------------------------------------------------------------------------------
_BUF_DTYPES = {16: (np.float32, 4), 4: (np.uint32, 1), 8: (np.uint16, 4), 64: (np.uint32, 16)}


#: HkRay / HkRayHit as numpy record types (Engine.cast_rays)
RAY_DTYPE = np.dtype([("origin", np.float32, 3), ("max_distance", np.float32), ("direction", np.float32, 3), ("exclude_instance", np.uint32)])
HIT_DTYPE = np.dtype([("distance", np.float32), ("instance", np.uint32), ("primitive", np.uint32), ("material", np.uint32),
                      ("barycentric", np.float32, 2), ("uv", np.float32, 2), ("normal", np.float32, 3), ("status", np.uint32)])
assert RAY_DTYPE.itemsize == 32 and HIT_DTYPE.itemsize == 48


def make_rays(origins, directions, max_distance=3.4028234663852886e38, exclude_instance=F.NO_INSTANCE):
    """A RAY_DTYPE array from (n, 3) origins and directions; max_distance / exclude_instance scalars or (n,) arrays."""
    o = np.asarray(origins, dtype=np.float32).reshape(-1, 3)
    r = np.zeros(len(o), dtype=RAY_DTYPE)
    r["origin"], r["direction"] = o, np.asarray(directions, dtype=np.float32).reshape(-1, 3)
    r["max_distance"], r["exclude_instance"] = max_distance, exclude_instance
    return r


def _present_formats():
    import torch

    return {"rgba16f": (F.FORMAT_RGBA16F, torch.float16), "rgba32f": (F.FORMAT_RGBA32F, torch.float32),
            "rgba8-srgb": (F.FORMAT_RGBA8_UNORM_SRGB, torch.uint8), "bgra8-srgb": (F.FORMAT_BGRA8_UNORM_SRGB, torch.uint8)}


def image_desc(im):
    """An HkImageDesc from dict(rgba=uint8[h][w][4], srgb, address_u, address_v, linear); the pixel array stays alive with the record."""
    a = np.ascontiguousarray(im["rgba"], dtype=np.uint8)
    assert a.ndim == 3 and a.shape[2] == 4
    d = F.HkImageDesc()
    d.rgba8, d.height, d.width = a.ctypes.data, a.shape[0], a.shape[1]
    d.is_srgb, d.filter_linear = int(im.get("srgb", True)), int(im.get("linear", True))
    d.address_u, d.address_v = im.get("address_u", F.ADDRESS_REPEAT), im.get("address_v", F.ADDRESS_REPEAT)
    d._pixels = a
    return d


def _texture_record(desc):
    """What Engine keeps of an uploaded texture: its size (read_texture) and its sampler (update_textures fills in what an item leaves out)."""
    return dict(width=desc.width, height=desc.height, srgb=bool(desc.is_srgb), address_u=desc.address_u, address_v=desc.address_v, filter=bool(desc.filter_linear))


_TEXEL_FORMATS = {"uint8": F.TEXELS_U8, "float16": F.TEXELS_F16, "float32": F.TEXELS_F32}


def texture_source(index, array, layout="hwc", origin=(0, 0), linear=False, sampler=None):
    """One HkTextureSource over `array` - a torch tensor or a numpy array of uint8 / float16 / float32, [h][w][c] (layout "hwc"),
    [c][h][w] ("chw") or [h][w] (grey), c = 1, 3 or 4 - read where it lies: pointer, strides and channel count come from the array, so a
    slice or an expanded (stride 0) array costs no copy.  sampler: None (the descriptor stays) or dict(srgb, address_u, address_v,
    filter), all four given."""
    is_torch = type(array).__module__.partition(".")[0] == "torch"
    fmt = _TEXEL_FORMATS.get(str(array.dtype).replace("torch.", ""))
    if fmt is None:
        raise TypeError(f"texels of dtype {array.dtype}: uint8, float16 or float32")
    elem = array.element_size() if is_torch else array.itemsize
    shape = tuple(array.shape)
    strides = tuple(s * elem for s in array.stride()) if is_torch else tuple(array.strides)
    if any(s < 0 for s in strides):
        raise ValueError("negative strides (a flipped array) are not supported: flip a copy")
    if len(shape) == 2:
        (h, w), (sy, sx), c, sc = shape, strides, 1, 0
    elif len(shape) == 3 and layout == "hwc":
        (h, w, c), (sy, sx, sc) = shape, strides
    elif len(shape) == 3 and layout == "chw":
        (c, h, w), (sc, sy, sx) = shape, strides
    else:
        raise ValueError(f"texels of shape {shape} in layout {layout!r}: [h][w][c] (\"hwc\"), [c][h][w] (\"chw\") or [h][w]")
    s = F.HkTextureSource()
    s.index, s.format, s.channels = index, fmt, c
    s.data = array.data_ptr() if is_torch else array.ctypes.data
    s.stride_x, s.stride_y, s.stride_c = sx, sy, sc
    (s.x0, s.y0), s.width, s.height = origin, w, h
    s.flags = (F.TEXTURE_LINEAR_SOURCE if linear else 0) | (F.TEXTURE_SET_SAMPLER if sampler is not None else 0)
    if sampler is not None:
        s.is_srgb, s.filter_linear = int(bool(sampler["srgb"])), int(bool(sampler["filter"]))
        s.address_u, s.address_v = sampler["address_u"], sampler["address_v"]
    return s


def encode_texels(array, layout="hwc", linear=False, texture_srgb=True):
    """hk_encode_texels: the bytes Engine.update_textures leaves for the same values, uint8[h][w][4] - `array` is a numpy array as in
    texture_source; texture_srgb is the texture's sRGB bit after the call.  Needs no GPU."""
    src = texture_source(0, array, layout, linear=linear)
    out = np.zeros((src.height, src.width, 4), np.uint8)
    F.api().call("encode_texels", C.byref(src), int(bool(texture_srgb)), out.ctypes.data)
    return out


def _fp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(F.f32))


def _morph_arrays(base_positions, base_normals, position_deltas, normal_deltas):
    """((n_vertices, n_targets), base positions, base normals, position deltas, normal deltas or None) of a morph set as contiguous float32"""
    bp = np.ascontiguousarray(base_positions, dtype=np.float32).reshape(-1, 3)
    bn = np.ascontiguousarray(base_normals, dtype=np.float32).reshape(-1, 3)
    dp = np.ascontiguousarray(position_deltas, dtype=np.float32)
    dp = dp.reshape(-1, len(bp), 3) if len(bp) else dp.reshape(0, 0, 3)
    dn = None if normal_deltas is None else np.ascontiguousarray(normal_deltas, dtype=np.float32).reshape(-1, len(bp), 3)
    if bn.shape != bp.shape or (dn is not None and dn.shape != dp.shape):
        raise ValueError("base normals must match base positions, normal deltas the position deltas")
    return (len(bp), len(dp)), bp, bn, dp, dn


def morph_vertices(base_positions, base_normals, position_deltas, normal_deltas, weights):
    """hk_morph_vertices: (positions, normals) a ("morph", index, weights) item leaves on the device for a set of these arrays
    (Engine.set_mesh_morph_targets) - base plus the targets whose weight is not zero, in ascending index.  Needs no GPU."""
    (nv, nt), bp, bn, dp, dn = _morph_arrays(base_positions, base_normals, position_deltas, normal_deltas)
    w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
    if len(w) != nt:
        raise ValueError(f"{nt} targets but {len(w)} weights")
    pos, nrm = np.empty_like(bp), np.empty_like(bn)
    F.api().call("morph_vertices", nv, nt, _fp(bp), _fp(bn), _fp(dp), _fp(dn), _fp(w), _fp(pos), _fp(nrm))
    return pos, nrm


def deform_items(items):
    """The HkMeshDeform table of Engine.deform_meshes' `items`, and the arrays it points into (to be kept alive over the call)."""
    table, keep = (F.HkMeshDeform * max(len(items), 1))(), []
    fp = lambda a: a.ctypes.data_as(C.POINTER(F.f32))
    for k, item in enumerate(items):
        kind, mesh = item[0], item[1]
        if kind == "skin":
            if len(item) != 3:
                raise ValueError('a skin item is ("skin", index, joints)')
            j = np.ascontiguousarray(item[2], dtype=np.float32).reshape(-1, 16)
            keep.append(j)
            table[k] = F.HkMeshDeform(mesh, F.DEFORM_SKIN, len(j), fp(j), None)
        elif kind == "morph":
            if len(item) != 3:
                raise ValueError('a morph item is ("morph", index, weights)')
            w = np.ascontiguousarray(item[2], dtype=np.float32).reshape(-1)
            keep.append(w)
            table[k] = F.HkMeshDeform(mesh, F.DEFORM_MORPH, len(w), fp(w), None)
        elif kind == "morph_skin":
            if len(item) != 4:
                raise ValueError('a morph + skin item is ("morph_skin", index, joints, weights)')
            j = np.ascontiguousarray(item[2], dtype=np.float32).reshape(-1, 16)
            w = np.ascontiguousarray(item[3], dtype=np.float32).reshape(-1)
            keep += [j, w]
            table[k] = F.HkMeshDeform(mesh, F.DEFORM_MORPH_SKIN, len(j), fp(j), fp(w))
        elif kind == "vertices":
            pos = np.ascontiguousarray(item[2], dtype=np.float32).reshape(-1, 3)
            nrm = None if len(item) < 4 or item[3] is None else np.ascontiguousarray(item[3], dtype=np.float32).reshape(-1, 3)
            if nrm is not None and nrm.shape != pos.shape:
                raise ValueError("normals must match positions")
            keep += [pos, nrm]
            table[k] = F.HkMeshDeform(mesh, F.DEFORM_VERTICES, len(pos), fp(pos), None if nrm is None else fp(nrm))
        else:
            raise ValueError(f"unknown deformation kind {kind!r}")
    return table, keep


def _item_arrays(item):
    return [a for a in item[2:4] if a is not None and not isinstance(a, dict)]


def _item_options(item):
    """the trailing dict of an item: ("vertices", index, positions, None, dict(recompute_normals=True))"""
    options = item[-1] if isinstance(item[-1], dict) else {}
    if set(options) - {"recompute_normals"}:
        raise ValueError(f"unknown item options {sorted(set(options) - {'recompute_normals'})}")
    return options


def _is_device_tensor(a):
    return type(a).__module__.partition(".")[0] == "torch" and bool(getattr(a, "is_cuda", False))


def deform_items_device(items, device):
    """The HkMeshDeformDevice table of Engine.deform_meshes' `items` when their arrays are torch tensors on cuda:`device`, and the tensors
    it points into.  float32 tensors whose rows are contiguous are named where they lie - pointer and row stride from the tensor, so a
    column slice state[:, 0:3] of a wider state tensor costs no copy; anything else is converted on the device first."""
    import torch

    def rows(t, width):
        if t.device.index != device:
            raise ValueError(f"the tensor lies on {t.device}, the context on cuda:{device}")
        t = t.reshape(-1, width) if t.dim() != 2 else t
        if t.shape[1] != width:
            raise ValueError(f"expected rows of {width} floats, not {tuple(t.shape)}")
        if t.dtype != torch.float32 or (len(t) > 1 and (t.stride(1) != 1 or t.stride(0) < width)) or (len(t) <= 1 and not t.is_contiguous()):
            t = t.to(torch.float32).contiguous()
        return t

    def weights(t):
        """morph weights: a contiguous float32 vector - a slice of a larger tensor is named where it lies"""
        if t.device.index != device:
            raise ValueError(f"the tensor lies on {t.device}, the context on cuda:{device}")
        t = t.reshape(-1)
        return t if t.dtype == torch.float32 and t.is_contiguous() else t.to(torch.float32).contiguous()

    table, keep = (F.HkMeshDeformDevice * max(len(items), 1))(), []
    for k, item in enumerate(items):
        kind, mesh = item[0], item[1]
        flags = F.DEFORM_RECOMPUTE_NORMALS if _item_options(item).get("recompute_normals") else 0
        if kind == "skin":
            if len(_item_arrays(item)) != 1:
                raise ValueError('a skin item is ("skin", index, joints)')
            j = rows(item[2], 16).contiguous()
            keep.append(j)
            table[k] = F.HkMeshDeformDevice(mesh, F.DEFORM_SKIN, len(j), j.data_ptr(), None, 0, 0, flags, 0)
        elif kind in ("morph", "morph_skin"):
            if len(_item_arrays(item)) != (1 if kind == "morph" else 2):
                raise ValueError('a morph item is ("morph", index, weights), a morph + skin item ("morph_skin", index, joints, weights)')
            w = weights(item[2] if kind == "morph" else item[3])
            if kind == "morph":
                keep.append(w)
                table[k] = F.HkMeshDeformDevice(mesh, F.DEFORM_MORPH, len(w), w.data_ptr(), None, 0, 0, flags, 0)
            else:
                j = rows(item[2], 16).contiguous()
                keep += [j, w]
                table[k] = F.HkMeshDeformDevice(mesh, F.DEFORM_MORPH_SKIN, len(j), j.data_ptr(), w.data_ptr(), 0, 0, flags, 0)
        elif kind == "vertices":
            pos = rows(item[2], 3)
            nrm = None if len(item) < 4 or item[3] is None or isinstance(item[3], dict) else rows(item[3], 3)
            if nrm is not None and nrm.shape != pos.shape:
                raise ValueError("normals must match positions")
            keep += [pos, nrm]
            table[k] = F.HkMeshDeformDevice(mesh, F.DEFORM_VERTICES, len(pos), pos.data_ptr(), None if nrm is None else nrm.data_ptr(),
                                            4 * pos.stride(0) if len(pos) > 1 else 0, 4 * nrm.stride(0) if nrm is not None and len(nrm) > 1 else 0, flags, 0)
        else:
            raise ValueError(f"unknown deformation kind {kind!r}")
    return table, keep


def mesh_sources_device(sources, device):
    """The HkMeshSource table of Engine.add_meshes' `sources` - {mesh_id: dict(positions=, normals=, uvs=None, indices=None)} of torch
    tensors on cuda:`device` - and the tensors it points into.  float32 tensors whose rows are contiguous are named where they lie, pointer
    and row stride from the tensor (a column slice state[:, 0:3] costs no copy, as in deform_items_device); indices are a contiguous int32 /
    uint32 tensor (another integer type is refused); any other float layout is converted on the device first - on torch's CURRENT stream,
    so Engine.add_meshes calls this under the producer's stream: the C call orders itself against that stream alone."""
    import torch

    def rows(t, width):
        if not _is_device_tensor(t) or t.device.index != device:
            raise ValueError(f"a source must be a torch tensor on cuda:{device}")
        t = t.reshape(-1, width) if t.dim() != 2 else t
        if t.shape[1] != width:
            raise ValueError(f"expected rows of {width} floats, not {tuple(t.shape)}")
        if t.dtype != torch.float32 or (len(t) > 1 and (t.stride(1) != 1 or t.stride(0) < width)) or (len(t) <= 1 and not t.is_contiguous()):
            t = t.to(torch.float32).contiguous()
        return t

    stride = lambda t: 4 * t.stride(0) if len(t) > 1 else 0
    table, keep = (F.HkMeshSource * max(len(sources), 1))(), []
    for k, (mesh_id, src) in enumerate(sources.items()):
        if set(src) - {"positions", "normals", "uvs", "indices"}:
            raise ValueError(f"unknown source arrays {sorted(set(src) - {'positions', 'normals', 'uvs', 'indices'})}")
        pos, nrm = rows(src["positions"], 3), rows(src["normals"], 3)
        uv = None if src.get("uvs") is None else rows(src["uvs"], 2)
        idx = src.get("indices")
        if idx is not None:
            if not _is_device_tensor(idx) or idx.device.index != device:
                raise ValueError(f"a source must be a torch tensor on cuda:{device}")
            if idx.dtype not in (torch.int32, torch.uint32):   # (a wider type would have to be narrowed, and a value >= 2^31 would wrap silently)
                raise ValueError(f"indices must be an int32 or uint32 tensor, not {idx.dtype}")
            idx = idx.reshape(-1)
            if not idx.is_contiguous():
                idx = idx.contiguous()
        keep += [pos, nrm, uv, idx]
        table[k] = F.HkMeshSource(int(mesh_id), 0, pos.data_ptr(), nrm.data_ptr(), None if uv is None else uv.data_ptr(), None if idx is None else idx.data_ptr(),
                                  stride(pos), stride(nrm), 0 if uv is None else stride(uv), 0)
    return table, keep


class Engine:
    """One context of the C ABI (`hk_ctx`).  `api` defaults to the product library."""
    _producer = None  # deform_meshes: a torch stream standing in for torch's legacy default stream (made at the first such call)
    _n_instances = None  # instances of the scene last uploaded / of the builder last given to set_instance_transforms (read_instance_transforms)
    _textures = None     # per uploaded texture its size and sampler (_texture_record): read_texture, update_textures

    def __init__(self, api=None, device=0, flags=0):
        self.api = api or F.api()
        self.ctx = C.c_void_p()
        self.api.call("create", device, flags | F.DEFAULT_CTX_FLAGS, C.byref(self.ctx))
        self.width = self.height = 0
        self.device = device
        self.owned = True
        self.generation = 0  # bumped by resize(): holders of device pointers / views compare it (distributed.BandRenderer)

    @classmethod
    def borrowed(cls, api, ctx):
        """An Engine over a context somebody else owns (hk_multi_context): never destroyed from here."""
        e = cls.__new__(cls)
        e.api, e.ctx, e.owned, e.generation, e.width, e.height, e.device = api, ctx, False, 0, 0, 0, None
        return e

    def close(self):
        if self.ctx and getattr(self, "owned", True):
            self.api.raw("destroy")(self.ctx)
        self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- Prepare stage
    def upload_scene(self, scene: SceneData):
        self.upload_textures(getattr(scene, "textures", []))
        scene.upload(self.api, self.ctx)
        self._n_instances = len(scene.instances)
        self._consumed(scene)

    def upload_instances(self, scene: SceneData):
        """Instance-level update of a scene whose meshes and materials are already uploaded."""
        scene.upload_instances(self.api, self.ctx)
        self._n_instances = len(scene.instances)
        self._consumed(scene)

    @staticmethod
    def _consumed(scene):
        """the context holds the instance set of the scene's builder (where the SceneData carries one): its origin list starts over"""
        builder = getattr(scene, "builder", None)
        if builder is not None and hasattr(builder, "take_origins"):
            builder.take_origins()

    def load_scene(self, builder, mode=F.TREE_SAH, textures=()):
        """hk_load_scene: the upload of a FINISHED builder whose deferred meshes (SceneBuilder.add_mesh(build_tree=False)) get their trees
        built on the device - F.TREE_SAH = the trees the host builds, F.TREE_LBVH = the quick Morton-order trees - and written back into
        the builder.  Returns the refreshed SceneData."""
        self.upload_textures(list(textures))
        self.api.call("load_scene", self.ctx, builder.h, mode)
        if hasattr(builder, "take_origins"):
            builder.take_origins()
        return builder.scene()

    def last_load(self):
        """(meshes built on the device, their triangles, kernel launches of the build, meshes completed on the host) of the last
        load_scene (test hook)."""
        out = (F.u32 * 4)()
        self.api.call("debug_last_load", self.ctx, out)
        return tuple(int(v) for v in out)

    def add_meshes(self, builder, mode=F.TREE_SAH, sources=None, producer_stream=None):
        """hk_add_meshes: the meshes added to the loaded, FINISHED `builder` since this context took its mesh level from it are appended to
        the device scene - deferred ones (SceneBuilder.add_mesh(build_tree=False)) get their trees built on the device and written back -
        without laying the scene out again.  Their instances follow through update_instances_on_device.  Returns nothing: the call's cost
        follows the new meshes, and builder.scene() - a copy of every array of the builder - would make it follow the scene.
        `sources` (hk_add_meshes_device): {mesh_id: dict(positions=, normals=, uvs=None, indices=None)} of torch tensors on the context's
        device for the meshes the builder declared by their counts (SceneBuilder.declare_mesh) - every such mesh exactly once.  Their
        records are assembled on the device and the builder gets the geometry back: afterwards it holds what add_mesh(build_tree=False) of
        the same values and this call would have left.  The context is ordered behind `producer_stream` (default: torch's current stream)
        and that stream behind the context's read of the tensors, which may be overwritten right after the call."""
        if sources is None:
            self.api.call("add_meshes", self.ctx, builder.h, mode)
            return
        import torch

        producer = torch.cuda.current_stream(self.device) if producer_stream is None else producer_stream
        with torch.cuda.stream(producer):   # (conversions of tensors that cannot be named where they lie run where the call orders itself)
            table, keep = mesh_sources_device(sources, self.device)
        self._producer_call(producer, lambda handle: self.api.call("add_meshes_device", self.ctx, builder.h, table, len(sources), mode, handle))

    def last_add_sources(self):
        """(sources taken from device memory, their triangles, kernel launches that assembled them, bytes of HkPrimitive / HkVertex records
        staged host to device) of the last add_meshes (test hook)."""
        out = (F.u32 * 4)()
        self.api.call("debug_last_add_sources", self.ctx, out)
        return tuple(int(v) for v in out)

    def last_add_source_times(self):
        """ms of the last add_meshes with sources: (the assembling launch between two events - only while F.DEBUG_OPT_ADD_SOURCE_TIMES is
        set, else 0 - the wait with the read-back, the builder's store) - hk_debug_last_add_source_times (measurement hook)."""
        out = (C.c_double * 3)()
        self.api.call("debug_last_add_source_times", self.ctx, out)
        return tuple(float(v) for v in out)

    def last_add(self):
        """(meshes built on the device, their triangles, kernel launches of the build, meshes whose trees the host had built, 1 if the scene
        moved to a larger allocation) of the last add_meshes (test hook)."""
        out = (F.u32 * 5)()
        self.api.call("debug_last_add", self.ctx, out)
        return tuple(int(v) for v in out)

    def remove_meshes(self, extents):
        """hk_remove_meshes: the meshes whose extents SceneBuilder.remove_mesh returned since the builder's last finish leave the device
        scene - the mesh level is compacted into a new, smaller allocation in one launch, behind the frames in flight, and the instance
        records are rebased.  Their instances must be gone already (update_instances_on_device).  Survivors are named by their new
        records afterwards (SceneBuilder.mesh_index after the finish, or rebase_mesh_index)."""
        extents = list(extents)
        arr = (F.HkMeshExtent * max(1, len(extents)))(*extents)
        self.api.call("remove_meshes", self.ctx, arr, len(extents))

    def last_remove(self):
        """(meshes removed, their triangles, kernel launches, runs per plane, path: 0 device compaction / 1 full layout, bytes moved) of
        the last remove_meshes (test hook)."""
        out = (C.c_uint64 * 6)()
        self.api.call("debug_last_remove", self.ctx, out)
        return tuple(int(v) for v in out)

    def last_remove_ms(self):
        """ms of the compaction launch of the last remove_meshes between two HIP events (measurement hook; waits for it)."""
        out = F.f32()
        self.api.call("debug_last_remove_ms", self.ctx, C.byref(out))
        return float(out.value)

    def last_add_times(self):
        """ms of the last add_meshes: (allocations of a relocation, its copy launch and switch, growth of the mirrors, staging + build +
        read-back) - hk_debug_last_add_times (measurement hook)."""
        out = (C.c_double * 4)()
        self.api.call("debug_last_add_times", self.ctx, out)
        return tuple(float(v) for v in out)

    def refit_instances(self, builder):
        """Instance motion on the device (hk_refit_scene_instances): the poses set on `builder` since the last upload / refit go to
        the GPU, which redoes the per-instance work and refits both trees.  Returns the number of instances that moved."""
        moved = C.c_uint32()
        self.api.call("refit_scene_instances", self.ctx, builder.h, C.byref(moved))
        return moved.value

    def update_instances_on_device(self, builder, mode=F.TREE_SAH):
        """Instances added / removed / re-materialed on `builder`: hk_update_scene_instances (host lays out the records, the device
        builds both trees)."""
        self.api.call("update_scene_instances", self.ctx, builder.h, mode)
        if hasattr(builder, "take_origins"):
            builder.take_origins()

    def change_instances(self, builder, mode=F.TREE_SAH):
        """Instances added / removed / re-materialed on `builder` in ANY state of the scene - after mesh deformations and device poses too,
        where update_instances_on_device is refused: hk_change_scene_instances (the host lays the level out, the device writes its own
        values over what the host's mirrors hold stale - survivors' poses, boxes, emitter records, alias tables - and builds both trees).
        The builder's origin list (SceneBuilder.origins) travels with the call and is reset to the identity once the call is accepted."""
        origins = np.array(builder.origins, dtype=np.uint32)
        self.api.call("change_scene_instances", self.ctx, builder.h, origins.ctypes.data_as(C.POINTER(F.u32)), len(origins), mode)
        if hasattr(builder, "take_origins"):
            builder.take_origins()
        self._n_instances = len(origins)

    def last_instance_change(self):
        """(kernel launches of the device path, instances carried over, new instances, bit 0: the scene moved to larger slots | bit 1: the
        call took update_instances_on_device's path) of the last change_instances - hk_debug_last_instance_change (test hook)."""
        out = (F.u32 * 4)()
        self.api.call("debug_last_instance_change", self.ctx, out)
        return tuple(int(v) for v in out)

    def update_materials(self, builder, mode=F.TREE_SAH):
        """Material edits on the device (hk_update_materials): the values set on `builder` (SceneBuilder.set_material) since the materials
        were last uploaded / updated.  Emitters that stay emitters are re-derived and the light tree refit in place; an emitter switched
        on or off takes the path of update_instances_on_device (trees built in `mode`).  In a frame that also moves instances call this
        before refit_instances.  Returns the number of material records that changed."""
        changed = C.c_uint32()
        self.api.call("update_materials", self.ctx, builder.h, mode, C.byref(changed))
        return changed.value

    def rebuild_trees(self, mode=F.TREE_SAH):
        """New instance tree and light tree over the current boxes, built on the device (hk_rebuild_scene_trees): F.TREE_SAH = the
        reference's own binned-SAH tree, F.TREE_LBVH = the quick Morton-order tree."""
        self.api.call("rebuild_scene_trees", self.ctx, mode)

    def update_mesh_vertices(self, mesh, positions, normals=None):
        """New positions (and normals, None = keep) of one uploaded mesh, written and refit on the device (hk_update_mesh_vertices)."""
        pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        nrm = None if normals is None else np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        if nrm is not None and nrm.shape != pos.shape:
            raise ValueError("normals must match positions")
        self.api.call("update_mesh_vertices", self.ctx, C.byref(mesh), len(pos), pos.ctypes.data_as(C.POINTER(F.f32)),
                      None if nrm is None else nrm.ctypes.data_as(C.POINTER(F.f32)))

    def set_mesh_skin(self, mesh, bind_positions, bind_normals, joint_indices, joint_weights):
        """Linear-blend skin of one uploaded mesh (hk_set_mesh_skin): bind pose, 4 joint indices (uint16) and 4 weights per vertex."""
        pos = np.ascontiguousarray(bind_positions, dtype=np.float32).reshape(-1, 3)
        nrm = np.ascontiguousarray(bind_normals, dtype=np.float32).reshape(-1, 3)
        idx = np.ascontiguousarray(joint_indices, dtype=np.uint16).reshape(-1, 4)
        w = np.ascontiguousarray(joint_weights, dtype=np.float32).reshape(-1, 4)
        if not (len(pos) == len(nrm) == len(idx) == len(w)):
            raise ValueError("bind positions, normals, joint indices and weights must have one row per vertex")
        fp = lambda a: a.ctypes.data_as(C.POINTER(F.f32))
        self.api.call("set_mesh_skin", self.ctx, C.byref(mesh), len(pos), fp(pos), fp(nrm), idx.ctypes.data_as(C.POINTER(C.c_uint16)), fp(w))

    def set_mesh_morph_targets(self, mesh, base_positions, base_normals, position_deltas, normal_deltas=None):
        """Morph targets (blend shapes) of one uploaded mesh, set once (hk_set_mesh_morph_targets): base positions and normals [v][3],
        position deltas [target][v][3] and normal deltas alike (None: the normals do not morph).  Per frame a ("morph", index, weights)
        or ("morph_skin", index, joints, weights) item of deform_meshes carries the weights alone."""
        arrays = _morph_arrays(base_positions, base_normals, position_deltas, normal_deltas)
        self.api.call("set_mesh_morph_targets", self.ctx, C.byref(mesh), *arrays[0], *[_fp(a) for a in arrays[1:]])

    def skin_mesh(self, mesh, joint_matrices):
        """Per frame: column-major 4x4 joint matrices (n x 16 floats); the device skins and refits (hk_skin_mesh)."""
        j = np.ascontiguousarray(joint_matrices, dtype=np.float32).reshape(-1, 16)
        self.api.call("skin_mesh", self.ctx, C.byref(mesh), j.ctypes.data_as(C.POINTER(F.f32)), len(j))

    def deform_meshes(self, items, producer_stream=None):
        """Many meshes deformed in one call (hk_deform_meshes): `items` is a list of ("vertices", index, positions, normals_or_None) and
        ("skin", index, joints) tuples - what update_mesh_vertices / skin_mesh take, mesh by mesh - and of ("morph", index, weights) and
        ("morph_skin", index, joints, weights) tuples for meshes with a morph set (set_mesh_morph_targets).  The device work is a fixed number of
        launches however many items there are; the result is what the single calls in item order would have left.
        Items whose arrays are torch tensors on the context's device take hk_deform_meshes_device: nothing is copied to the host, the
        context is ordered behind `producer_stream` (a torch stream; default: torch's current stream) by an event, and that stream behind
        the context's last read of the tensors, so they may be overwritten in stream order right after the call - there is no host wait.
        Such a "vertices" item may end in dict(recompute_normals=True) (with normals None): the device recomputes the vertex normals
        from the new positions (SceneBuilder.recompute_mesh_normals is the host's mirror).  numpy items go through hk_deform_meshes."""
        on_device = [_is_device_tensor(a) for item in items for a in _item_arrays(item)]
        if not any(on_device):
            if any(_item_options(item).get("recompute_normals") for item in items):
                raise ValueError("recompute_normals needs items whose arrays are torch tensors on the context's device")
            table, keep = deform_items([tuple(a for a in item if not isinstance(a, dict)) for item in items])
            self.api.call("deform_meshes", self.ctx, table, len(items))
            return
        if not all(on_device):
            raise ValueError("the items of one batch are either all torch tensors on the context's device or all host arrays")
        table, keep = deform_items_device(items, self.device)
        self._producer_call(producer_stream, lambda handle: self.api.call("deform_meshes_device", self.ctx, table, len(items), handle))

    def _producer_call(self, producer_stream, call):
        """call(handle of the stream the C call orders itself against): `producer_stream` (a torch stream; None: torch's current stream),
        or a stream of the engine's own standing in for torch's legacy default stream - whose handle 0 the C call reads as "the caller has
        ordered itself" - ordered behind it before the call and in front of it after (events, no host wait)."""
        import torch

        current = torch.cuda.current_stream(self.device) if producer_stream is None else producer_stream
        if current.cuda_stream:
            return call(current.cuda_stream)
        if self._producer is None:
            self._producer = torch.cuda.Stream(self.device)
        self._producer.wait_stream(current)
        out = call(self._producer.cuda_stream)
        current.wait_stream(self._producer)
        return out

    def set_instance_transforms(self, builder, models, ids=None, producer_stream=None, status=None):
        """Instance poses from device memory (hk_set_instance_transforms_device).  `models`: a float32 torch tensor (n, 4, 4) or (n, 16) on
        the context's device, pose k = 16 floats in column-major order (what SceneBuilder.set_instance_transform takes), rows at any
        stride - a column slice state[:, :16] of a wider state tensor is read where it lies.  `ids` (a host sequence) names the instance
        of every row; None: rows 0 .. n - 1 are instances 0 .. n - 1.  Which instance moved is decided on the device; an instance not
        named is at rest.  `status` (a 1-element int32 / uint32 tensor on the device, optional) receives 1 + the highest instance id
        whose pose was not finite or singular - such an instance keeps its pose - or 0, in stream order.  The context is ordered behind
        `producer_stream` (default: torch's current stream) and that stream behind the context's read of `models`, by events: there is
        no host wait, and the tensor may be overwritten right after the call.  Afterwards refit_instances and
        update_instances_on_device are refused until read_instance_transforms + SceneBuilder.set_instance_transform +
        upload_instances bring the poses back to the host."""
        if not _is_device_tensor(models):
            raise TypeError("models must be a torch tensor on the context's device (host poses go through SceneBuilder.set_instance_transform and refit_instances)")
        import torch

        if models.device.index != self.device:
            raise ValueError(f"the tensor lies on {models.device}, the context on cuda:{self.device}")
        if models.dim() == 3 and tuple(models.shape[1:]) == (4, 4):
            if len(models) and (models.stride(2) != 1 or models.stride(1) != 4):
                models = models.contiguous()
            models = models.as_strided((len(models), 16), (models.stride(0) if len(models) else 16, 1), models.storage_offset())
        if models.dim() != 2 or models.shape[1] != 16:
            raise ValueError(f"expected poses of shape (n, 4, 4) or (n, 16), not {tuple(models.shape)}")
        if models.dtype != torch.float32 or (len(models) > 1 and (models.stride(1) != 1 or models.stride(0) < 16)) or (len(models) <= 1 and not models.is_contiguous()):
            models = models.to(torch.float32).contiguous()
        n = len(models)
        id_array = None
        if ids is not None:
            id_array = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
            if len(id_array) != n:
                raise ValueError(f"{len(id_array)} ids for {n} poses")
        if status is not None and (not _is_device_tensor(status) or status.numel() < 1 or status.element_size() != 4):
            raise TypeError("status must be a 4-byte integer tensor on the context's device")
        stride = 4 * models.stride(0) if n > 1 else 64
        self._producer_call(producer_stream, lambda handle: self.api.call(
            "set_instance_transforms_device", self.ctx, builder.h, None if id_array is None else id_array.ctypes.data_as(C.POINTER(F.u32)), n, models.data_ptr(), stride, handle,
            None if status is None else status.data_ptr()))
        p, count = C.POINTER(F.HkInstance)(), F.u32()
        if self.api.raw("scene_builder_instances")(builder.h, C.byref(p), C.byref(count)) == F.HK_OK:
            self._n_instances = count.value   # (the call has checked it against the scene's)

    def read_instance_transforms(self, n=None):
        """The poses the device holds, float32 (n, 16), column-major (hk_read_instance_transforms; waits for the context's streams): the
        way back after set_instance_transforms.  `n`: the scene's instance count; None: the count of the scene last uploaded through
        this engine or of the builder last given to set_instance_transforms."""
        count = self._n_instances if n is None else int(n)
        if count is None:
            raise ValueError("the engine has not seen the scene's instance count: pass n")
        out = np.zeros((max(count, 1), 16), np.float32)
        self.api.call("read_instance_transforms", self.ctx, out.ctypes.data_as(C.POINTER(F.f32)), count)
        return out[:count]

    def last_pose(self):
        """(kernel launches of the last set_instance_transforms, 1 if it copied mesh boxes to the device) - hk_debug_last_pose (test hook)."""
        out = (F.u32 * 2)()
        self.api.call("debug_last_pose", self.ctx, out)
        return tuple(int(v) for v in out)

    def last_deform(self):
        """(items, vertices, triangles, enqueues of the call, launches of the last flush, launches of the last wide-record derivation) -
        hk_debug_last_deform (test hook)."""
        out = (F.u32 * 6)()
        self.api.call("debug_last_deform", self.ctx, out)
        return tuple(int(v) for v in out)

    def set_mesh_motion_vectors(self, mesh, enabled=True):
        """Per-vertex motion vectors for one deforming mesh, on or off (hk_set_mesh_motion_vectors): the device keeps the mesh's previous
        local positions (+16 B per vertex) and a pass behind the primary rays writes velocity_uv.xy of its pixels from them, in every
        frame that follows a deformation of the mesh.  Off by default: velocity is then the reference's rigid formula."""
        self.api.call("set_mesh_motion_vectors", self.ctx, C.byref(mesh), 1 if enabled else 0)

    def last_motion(self):
        """(launches of the motion pass in the last frame, meshes live in it, pixels rewritten - counted only with F.DEBUG_OPT_MOTION_COUNT
        set) - hk_debug_last_motion (test hook)."""
        out = (F.u32 * 3)()
        self.api.call("debug_last_motion", self.ctx, out)
        return tuple(int(v) for v in out)

    def rebuild_mesh_tree(self, mesh, mode=F.TREE_SAH):
        """A new tree over the current triangles of one uploaded mesh, built on the device in place (hk_rebuild_mesh_tree): F.TREE_SAH = the
        tree SceneBuilder.rebuild_mesh_tree builds, F.TREE_LBVH = the quick Morton-order tree.  Later deformations refit the new shape."""
        self.api.call("rebuild_mesh_tree", self.ctx, C.byref(mesh), mode)

    def read_mesh_nodes(self):
        """(nodes, count, orderings): the mesh-level node array as the device holds it, every ordering (test hook)."""
        n, o = F.u32(), F.u32()
        self.api.call("debug_read_mesh_nodes", self.ctx, None, 0, C.byref(n), C.byref(o))
        out = (F.HkNode * max(1, n.value * o.value))()
        self.api.call("debug_read_mesh_nodes", self.ctx, out, n.value * o.value, C.byref(n), C.byref(o))
        return out, n.value, o.value

    def read_emitters(self):
        """(records float32[n][8]: position xyz, radius, surface area, instance / alias offset / alias count as u32 bits; alias float32[m][2]:
        probability, index bits) as the device holds them (test hook)."""
        n, m = F.u32(), F.u32()
        self.api.call("debug_read_emitters", self.ctx, None, 0, C.byref(n), None, 0, C.byref(m))
        rec, al = np.zeros((max(1, n.value), 8), np.float32), np.zeros((max(1, m.value), 2), np.float32)
        fp = lambda a: a.ctypes.data_as(C.POINTER(F.f32))
        self.api.call("debug_read_emitters", self.ctx, fp(rec), n.value, C.byref(n), fp(al), m.value, C.byref(m))
        return rec[:n.value], al[:m.value]

    def read_mesh_geometry(self, mesh):
        """dict(positions, normals: float32[n][3]; triangles: float32[t][3][4] - v0, v1, v2 with the vertex-index words as float bits;
        box: float32[2][3]) of one mesh deformed on this context, as the device holds it (test hook)."""
        nv, nt = F.u32(), F.u32()
        self.api.call("debug_read_mesh_geometry", self.ctx, C.byref(mesh), None, None, 0, None, 0, None, C.byref(nv), C.byref(nt))
        pos, nrm = np.zeros((max(1, nv.value), 4), np.float32), np.zeros((max(1, nv.value), 4), np.float32)
        tri, box = np.zeros((max(1, nt.value), 3, 4), np.float32), np.zeros((2, 3), np.float32)
        fp = lambda a: a.ctypes.data_as(C.POINTER(F.f32))
        self.api.call("debug_read_mesh_geometry", self.ctx, C.byref(mesh), fp(pos), fp(nrm), nv.value, fp(tri), nt.value, fp(box), C.byref(nv), C.byref(nt))
        return dict(positions=pos[:nv.value, :3], normals=nrm[:nv.value, :3], triangles=tri[:nt.value], box=box)

    def read_trees(self, n_instance_nodes, n_emissive_nodes):
        """(instance_nodes, emissive_nodes) as the device holds them, in the reference layout (test hook)."""
        a, b = (F.HkNode * max(1, n_instance_nodes))(), (F.HkNode * max(1, n_emissive_nodes))()
        self.api.call("debug_read_trees", self.ctx, a, n_instance_nodes, b, n_emissive_nodes)
        return (F.HkNode * n_instance_nodes).from_buffer_copy(bytes(a)[:n_instance_nodes * C.sizeof(F.HkNode)]), \
               (F.HkNode * n_emissive_nodes).from_buffer_copy(bytes(b)[:n_emissive_nodes * C.sizeof(F.HkNode)])

    def upload_textures(self, images):
        """images: list of dict(rgba=uint8[h][w][4], srgb=bool, address_u/address_v=F.ADDRESS_*, linear=bool) -
        the `textures` / `samplers` binding arrays (mod.rs:760-782).  Material *_texture ids index this list."""
        one = [image_desc(im) for im in images]   # (each keeps its pixel array alive until the call has copied it)
        descs = (F.HkImageDesc * max(len(images), 1))(*one)
        self.api.call("upload_textures", self.ctx, descs, len(images))
        self._textures = [_texture_record(d) for d in one]

    def update_texture(self, index, image):
        """New texels and sampler of ONE uploaded texture of the same size (hk_update_texture), in place and without a host wait; `image`
        as in upload_textures."""
        desc = image_desc(image)
        self.api.call("update_texture", self.ctx, index, C.byref(desc))
        if self._textures is not None and index < len(self._textures):
            self._textures[index] = _texture_record(desc)

    def update_textures(self, items, producer_stream=None):
        """Texture edits from device memory, many per call (hk_update_textures_device): one kernel launch however many items there are,
        nothing is copied to the host and there is no host wait.  Each item is a dict: `index` (an uploaded texture); `tensor`, a torch
        uint8 / float16 / float32 tensor on the context's device, [h][w][c] with layout="hwc" (the default), [c][h][w] with "chw" or
        [h][w] (grey), c = 1, 3 or 4, read where it lies (a slice or an expanded tensor costs no copy); optional origin=(x0, y0) of the
        rectangle it fills (default: the corner; the tensor's size is the rectangle's); optional linear=True: a float tensor holds LINEAR
        light and the rgb of an sRGB texture are encoded (HK_TEXTURE_LINEAR_SOURCE); optional srgb, address_u, address_v, filter: a new
        sampler - those not given stay what the texture has.  uint8 is taken as it is, floats are the encoded value in [0, 1].
        The context is ordered behind `producer_stream` (a torch stream; default: torch's current stream) and that stream behind the
        context's read of the tensors, by events: they may be overwritten right after the call.  encode_texels is the host's twin."""
        if self._textures is None:
            raise ValueError("the engine has not uploaded textures (upload_textures)")
        table, keep = (F.HkTextureSource * max(len(items), 1))(), []
        samplers = [dict(t) for t in self._textures]
        for k, item in enumerate(items):
            tensor, index = item["tensor"], int(item["index"])
            if not _is_device_tensor(tensor):
                raise TypeError("tensor must be a torch tensor on the context's device (host texels go through update_texture)")
            if tensor.device.index != self.device:
                raise ValueError(f"the tensor lies on {tensor.device}, the context on cuda:{self.device}")
            if not 0 <= index < len(samplers):
                raise ValueError(f"texture {index} of {len(samplers)}")
            sampler = None
            if any(key in item for key in ("srgb", "address_u", "address_v", "filter")):
                sampler = samplers[index]
                sampler.update({key: item[key] for key in ("srgb", "address_u", "address_v", "filter") if key in item})
            table[k] = texture_source(index, tensor, item.get("layout", "hwc"), item.get("origin", (0, 0)), bool(item.get("linear", False)), sampler)
            keep.append(tensor)   # (alive until the call has returned: the producer stream is ordered behind the read by then)
        self._producer_call(producer_stream, lambda handle: self.api.call("update_textures_device", self.ctx, table, len(items), handle))
        for record, new in zip(self._textures, samplers):
            record.update(new)

    def read_texture(self, index):
        """The texels the device holds of one texture, uint8[h][w][4] (hk_read_texture; waits for the context's streams): the way back
        after update_textures."""
        if self._textures is None or not 0 <= index < len(self._textures):
            raise ValueError(f"texture {index}: the engine has uploaded {0 if self._textures is None else len(self._textures)}")
        out = np.zeros((self._textures[index]["height"], self._textures[index]["width"], 4), np.uint8)
        self.api.call("read_texture", self.ctx, index, out.ctypes.data, out.size)
        return out

    def last_texture_update(self):
        """(items, kernel launches, texels written) of the last update_textures - hk_debug_last_texture_update (test hook)."""
        out = (F.u32 * 3)()
        self.api.call("debug_last_texture_update", self.ctx, out)
        return tuple(int(v) for v in out)

    def upload_noise(self, noise=None):
        noise = load_noise() if noise is None else np.ascontiguousarray(noise, dtype=np.uint8)
        self.api.call("upload_noise", self.ctx, noise.ctypes.data, noise.size)

    def resize(self, width, height, upscale_ratio=1.0):
        self.api.call("resize", self.ctx, width, height, upscale_ratio)
        self.width, self.height = width, height
        self._bounds = None   # (hk_resize drops an explicit band split: it was in rows of the old render image)
        self.generation += 1  # every buffer was freed and reallocated: device pointers / views of an older generation are dead

    # -- per frame
    def frame_begin(self, frame, view, previous_view, lights):
        self.api.call("frame_begin", self.ctx, C.byref(frame), C.byref(view), C.byref(previous_view), C.byref(lights))

    def set_view_options(self, taa, upscale_kind, upscale_sharpness=0.0):
        self.api.call("set_view_options", self.ctx, taa, upscale_kind, upscale_sharpness)

    def pass_run(self, pass_id, arg=0, row_begin=0, row_end=0):
        self.api.call("pass_run", self.ctx, pass_id, arg, row_begin, row_end)

    def frame_stage(self, stage, settings_c, flags=0):
        self.api.call("frame_stage", self.ctx, stage, C.byref(settings_c), flags)

    def frame_render(self, frame, view, previous_view, lights, settings_c, flags=0):
        self.api.call("frame_render", self.ctx, C.byref(frame), C.byref(view), C.byref(previous_view), C.byref(lights), C.byref(settings_c), flags)

    def wait(self):
        self.api.call("frame_wait", self.ctx)

    def set_band(self, index, count):
        self.api.call("set_band", self.ctx, index, count)
        self._band = (index, count)

    def band_count(self):
        if "get_band" in self.api._fns:
            n = F.u32(0)
            self.api.call("get_band", self.ctx, None, C.byref(n))
            return n.value
        return getattr(self, "_band", (0, 1))[1]

    def set_band_bounds(self, bounds=None):
        """hk_set_band_bounds: band i renders scaled render rows [bounds[i], bounds[i + 1]); None = the equal split."""
        self._bounds = None if bounds is None else [int(b) for b in bounds]
        if bounds is None:
            self.api.call("set_band_bounds", self.ctx, None, 0)
            return
        arr = (C.c_uint32 * len(bounds))(*[int(b) for b in bounds])
        self.api.call("set_band_bounds", self.ctx, arr, len(bounds))

    def band_bounds(self):
        """hk_get_band_bounds: the split in force (band_count + 1 scaled render rows), explicit or equal."""
        n = self.band_count() + 1
        if "get_band_bounds" not in self.api._fns:   # (the oracle behind the same table)
            return getattr(self, "_bounds", None)
        out = (C.c_uint32 * n)()
        self.api.call("get_band_bounds", self.ctx, out, n)
        return [int(x) for x in out]

    def balance_bands(self, min_rows=0):
        """hk_balance_bands (after frame_begin): ray-cast the whole frame's primary rays, count geometry pixels per row, split the
        render rows by cost and keep the split.  Returns the boundaries - the same on every rank that does this for the frame."""
        _w, rh, _b = self.buffer_info(F.BUF_TONE_MAPPED)
        n = self.band_count() + 1
        if "balance_bands" in self.api._fns:
            out = (C.c_uint32 * n)()
            self.api.call("balance_bands", self.ctx, min_rows, out, n)
            return [int(x) for x in out]
        # (a library without the composite - the oracle behind the same ctypes table in the CPU tests: the same three steps)
        from .distributed import balanced_band_bounds

        if n == 2:
            return [0, rh]
        self.pass_run(F.PASS_PREPASS)
        w, _h, _b = self.buffer_info(F.BUF_POSITION)
        bounds = balanced_band_bounds(self.row_costs(), w, rh, n - 1, max(1, min(min_rows or 8, rh // (n - 1))), 0.25)   # (the CPU test scenes are LDS-sized)
        self.set_band_bounds(bounds)
        return bounds

    def migrate_bands(self, new_bounds, next_frame_number, settings_c):
        """hk_migrate_bands (needs a communicator): the history rows that change owner travel as one RCCL exchange, then the new split is
        set.  Every rank calls it with the same arguments between two frames.  new_bounds None = the equal split."""
        if new_bounds is None:
            self.api.call("migrate_bands", self.ctx, None, 0, int(next_frame_number), C.byref(settings_c))
        else:
            arr = (C.c_uint32 * len(new_bounds))(*[int(b) for b in new_bounds])
            self.api.call("migrate_bands", self.ctx, arr, len(new_bounds), int(next_frame_number), C.byref(settings_c))

    def band_time_ms(self):
        """hk_band_time_ms: the band's own GPU time (stage TEMPORAL + stage SPATIAL, without the waits for its neighbours' halos) in the
        last frame rendered with F.FRAME_TIME_BAND."""
        ms = C.c_float()
        self.api.call("band_time_ms", self.ctx, C.byref(ms))
        return float(ms.value)

    def row_costs(self):
        """hk_row_costs: geometry pixels per full-size row of the frame most recently begun (numpy uint32[height])."""
        _w, h, _b = self.buffer_info(F.BUF_POSITION)
        out = np.zeros(h, dtype=np.uint32)
        self.api.call("row_costs", self.ctx, out.ctypes.data_as(C.POINTER(C.c_uint32)), h)
        return out

    # -- buffers
    def buffer_info(self, buf):
        w, h, bpp = F.u32(), F.u32(), F.u32()
        self.api.call("buffer_info", self.ctx, buf, C.byref(w), C.byref(h), C.byref(bpp))
        return w.value, h.value, bpp.value

    def _buffer_layout(self, buf):
        w, h, bpp = self.buffer_info(buf)
        if buf in (F.BUF_DEPTH_GRADIENT, F.BUF_INSTANCE_MATERIAL):
            dt, k = np.float32, 2
        elif bpp == 4 and buf != F.BUF_NORMAL:
            dt, k = np.float32, 1
        else:
            dt, k = _BUF_DTYPES[bpp]
        return h, w, k, dt

    def read(self, buf):
        """Raw contents as a numpy array [h, w, k] (f32 for 16/8-byte float formats, u16 for rgba16f, u32 otherwise)."""
        h, w, k, dt = self._buffer_layout(buf)
        out = np.empty((h, w, k), dtype=dt)
        self.api.call("read_buffer", self.ctx, buf, out.ctypes.data, out.nbytes)
        return out

    def shape_buffer(self, buf, raw_bytes):
        """Raw bytes of `buf` (e.g. from hk_multi_read_buffer) as the array Engine.read would return."""
        h, w, k, dt = self._buffer_layout(buf)
        return np.frombuffer(raw_bytes, dtype=dt).reshape(h, w, k).copy()

    def read_f16(self, buf):
        return self.read(buf).view(np.float16).astype(np.float32)

    def write(self, buf, array):
        a = np.ascontiguousarray(array)
        self.api.call("write_buffer", self.ctx, buf, a.ctypes.data, a.nbytes)

    def device_ptr(self, buf):
        p, n = C.c_void_p(), C.c_size_t()
        self.api.call("device_ptr", self.ctx, buf, C.byref(p), C.byref(n))
        return p.value, n.value

    def allocated_bytes(self, buf):
        return self.device_ptr(buf)[1]

    # -- present (the reference's OverlayNode)
    def present_into(self, settings_c, frame_flags, device_ptr, width, height, pitch_bytes, fmt, flags=0, clear=None, rows=None):
        """hk_present: rows of a host-owned target in device memory.  Asynchronous, like frame_render; wait() returns once it is written."""
        t = F.HkPresentTarget(C.c_void_p(device_ptr), width, height, pitch_bytes, fmt, flags)
        if clear is not None:
            t.clear[:] = [float(v) for v in clear]
        y0, y1 = (0, height) if rows is None else rows
        self.api.call("present", self.ctx, C.byref(settings_c), frame_flags, C.byref(t), y0, y1)

    def present(self, settings, *, antialias, format="rgba16f", hdr=False, clear=None, out=None, rows=None, wait=True):
        """The frame last rendered as the camera's view target receives it (OverlayNode, overlay.rs:311-395): NaN texels replaced by
        the albedo, the tone map undone for an HDR target (`hdr`), alpha-blended over `clear` (four linear floats) or over what `out`
        holds (`clear=None`), in the target's format - "rgba16f", "rgba32f", "rgba8-srgb" or "bgra8-srgb".  Returns a torch tensor
        [H][W][4] (float16 / float32 / uint8) on the context's device: `out`, or a new one of the final image's size (zeros
        under clear=None).  The kernel writes `out.data_ptr()`; nothing passes through the host.  `rows` = (begin, end) presents
        those rows only.  A new tensor has the size of the final image of the frame last rendered with these settings.
        Synchronisation: torch and the context enqueue on different streams and share no event, so this call first waits on the
        host for torch's current stream (whatever torch still has in flight on `out`), and by default (wait=True) for the present
        itself, so that the tensor returned is safe to read from torch.  wait=False leaves the present enqueued, ordered against
        the context's later frames inside the library (hk_present): call wait() before torch touches the tensor."""
        import torch

        fmt, dtype = _present_formats()[format]
        sc = settings.to_c() if hasattr(settings, "to_c") else settings
        frame_flags = F.FRAME_ANTIALIAS if antialias else 0
        if out is None:
            if getattr(self, "device", None) is None:
                raise ValueError("present() on a borrowed context needs `out`")
            w, h, _ = self.buffer_info(self.api.final_buffer(sc, frame_flags))   # (as the frame last rendered left it: render with THESE settings)
            out = (torch.zeros if clear is None else torch.empty)((h, w, 4), dtype=dtype, device=torch.device("cuda", self.device))
        device = out.device
        if getattr(self, "device", None) is not None and device.type == "cuda" and device.index != self.device:
            raise ValueError(f"present(): `out` lives on {device}, the context on cuda:{self.device}")
        if out.dtype != dtype or out.dim() != 3 or out.shape[2] != 4 or out.stride(2) != 1 or out.stride(1) != 4 or device.type != "cuda":
            raise ValueError(f"present(format={format!r}) needs a {dtype} tensor [H][W][4] with contiguous pixels in device memory")
        torch.cuda.current_stream(device).synchronize()      # (what torch still has in flight on `out` comes first)
        flags = (F.PRESENT_HDR if hdr else 0) | (F.PRESENT_CLEAR if clear is not None else 0)
        self.present_into(sc, frame_flags, out.data_ptr(), out.shape[1], out.shape[0], out.stride(0) * out.element_size(), fmt, flags, clear, rows)
        if wait:
            self.wait()
        return out

    # -- ray queries (picking, line of sight, probe rays)
    def cast_rays(self, rays, *, any_hit=False, attributes=False, stackless=False, out=None, wait=True):
        """hk_cast_rays / hk_cast_rays_device: one HkRayHit per HkRay, against the scene this context holds (no resize, no frame).
        `rays`: a numpy array viewable as (n, 8) float32 - origin xyz, max_distance, direction xyz, exclude_instance as BITS - or a
        structured array of RAY_DTYPE (make_rays builds one); returns a structured numpy array of HIT_DTYPE (`out`, if given).
        A torch tensor of n x 32 bytes in device memory goes through hk_cast_rays_device without a copy: torch's current stream
        is synchronised first, the context is waited for afterwards (unless wait=False: call wait() before torch reads), and the
        result is a uint8 tensor [n][48] (`out`, or a new one) - view it as float32 / int32 columns as needed.
        any_hit: occlusion only (status; identity and distance are not promised).  attributes: also material, uv, normal.
        stackless: never the wide walk (F.RAYS_STACKLESS)."""
        flags = (F.RAYS_ANY if any_hit else 0) | (F.RAYS_ATTRIBUTES if attributes else 0) | (F.RAYS_STACKLESS if stackless else 0)
        if not isinstance(rays, np.ndarray) and hasattr(rays, "data_ptr"):
            import torch

            if rays.device.type != "cuda" or not rays.is_contiguous() or (rays.numel() * rays.element_size()) % 32:
                raise ValueError("cast_rays(): a contiguous tensor of n x 32 bytes in device memory is needed")
            n = rays.numel() * rays.element_size() // 32
            if out is None:
                out = torch.empty((n, 48), dtype=torch.uint8, device=rays.device)
            if out.device != rays.device or not out.is_contiguous() or out.numel() * out.element_size() != n * 48:
                raise ValueError("cast_rays(): `out` must be a contiguous tensor of n x 48 bytes on the rays' device")
            torch.cuda.current_stream(rays.device).synchronize()
            self.api.call("cast_rays_device", self.ctx, C.c_void_p(rays.data_ptr()), n, flags, C.c_void_p(out.data_ptr()))
            if wait:
                self.wait()
            return out
        r = np.ascontiguousarray(rays)
        if r.dtype != RAY_DTYPE:
            if r.dtype.itemsize != 4 or r.ndim != 2 or r.shape[1] != 8:
                raise ValueError("cast_rays(): rays must be (n, 8) of a 4-byte type or a structured array of RAY_DTYPE")
            r = r.view(RAY_DTYPE).reshape(-1)
        r = r.reshape(-1)
        if out is None:
            out = np.zeros(len(r), dtype=HIT_DTYPE)
        if out.dtype != HIT_DTYPE or out.shape != (len(r),) or not out.flags.c_contiguous:
            raise ValueError("cast_rays(): `out` must be a contiguous HIT_DTYPE array with one record per ray")
        self.api.call("cast_rays", self.ctx, C.cast(C.c_void_p(r.ctypes.data), C.POINTER(F.HkRay)), len(r), flags,
                      C.cast(C.c_void_p(out.ctypes.data), C.POINTER(F.HkRayHit)))
        return out

    # -- halo exchange inside the library (one process per GPU; bevy-hikari_amd/distributed.py does the rendezvous)
    def comm_available(self):
        """hk_comm_available as (ok, reason): never raises, so that every rank reaches the agreement step."""
        try:
            self.api.call("comm_available", self.ctx)
            return True, ""
        except Exception as err:  # HikariError from the library; KeyError / AttributeError behind a library without RCCL (the oracle)
            return False, repr(err)

    def comm_unique_id(self):
        ident = (C.c_uint8 * 128)()
        self.api.call("comm_unique_id", ident)
        return bytes(ident)

    def comm_init(self, rank, n_ranks, ident):
        buf = (C.c_uint8 * 128).from_buffer_copy(ident)
        self.api.call("comm_init", self.ctx, rank, n_ranks, buf)

    def comm_set_history_rows(self, rows):
        self.set_history_rows(rows)

    def set_history_rows(self, rows=F.HISTORY_AUTO):
        """hk_set_history_rows: rows of last frame's reservoirs a band fetches from its neighbours before TEMPORAL (and, doubled,
        of the parked scatter stores before SPATIAL).  F.HISTORY_AUTO (the default of a context): derived per frame."""
        self.api.call("set_history_rows", self.ctx, int(rows))

    def history_rows(self):
        """hk_history_rows: the count in force for the frame most recently begun (0 for a single band or a static view)."""
        n = F.u32(0)
        self.api.call("history_rows", self.ctx, C.byref(n))
        return n.value

    def scene_bounds(self):
        mn, mx = (F.f32 * 3)(), (F.f32 * 3)()
        self.api.call("scene_bounds", self.ctx, mn, mx)
        return list(mn), list(mx)

    def comm_gather(self, buffer, root=0):
        """hk_comm_gather: rank `root` collects every other rank's rows of `buffer` (RCCL, on the context's stream)."""
        self.api.call("comm_gather", self.ctx, buffer, root)

    def debug_comm_loopback(self, src_buffer, dst_buffer, row_begin, row_end, overlapped=False):
        """hk_debug_comm_loopback (hikari_hip_debug.h): rows of one buffer to the same rows of another through ncclSend / ncclRecv
        to the context's own rank, on the context's stream."""
        self.api.call("debug_comm_loopback", self.ctx, src_buffer, dst_buffer, row_begin, row_end, 1 if overlapped else 0)

    def comm_destroy(self):
        self.api.call("comm_destroy", self.ctx)

    def stats(self):
        s = F.HkStats()
        self.api.call("get_stats", self.ctx, C.byref(s))
        return s

    def reset_stats(self):
        self.api.call("reset_stats", self.ctx)

    def stream(self):
        """The HIP stream the context enqueues on (hk_stream), as an integer handle."""
        h = C.c_void_p()
        self.api.call("stream", self.ctx, C.byref(h))
        return h.value or 0

    def set_stream(self, hip_stream_ptr):
        """Run all subsequent work on a host-owned HIP stream (e.g. torch.cuda.current_stream().cuda_stream)."""
        self.api.call("set_stream", self.ctx, C.c_void_p(hip_stream_ptr))

    def set_timing_mask(self, mask):
        self.api.call("set_timing_mask", self.ctx, mask)

    def indirect_schedule(self):
        """'fused' or 'wavefront': the schedule indirect_lit_ambient takes for the frame most recently begun (HK_CTX_WAVEFRONT)."""
        v = C.c_uint32()
        self.api.call("indirect_schedule", self.ctx, C.byref(v))
        return "wavefront" if v.value else "fused"

    def traversal_mode(self):
        """('reference' | 'threaded' | 'one-level', stored direction orderings): hk_traversal_mode."""
        v, n = C.c_uint32(), C.c_uint32()
        self.api.call("traversal_mode", self.ctx, C.byref(v), C.byref(n))
        return ("reference", "threaded", "one-level")[v.value & 0xFF], n.value

    def wide_walk(self):
        """True when the closest-hit walks of the uploaded scene take the wide records (HK_TRAVERSAL_WIDE; HK_CTX_NO_WIDE_WALK)."""
        v = C.c_uint32()
        self.api.call("traversal_mode", self.ctx, C.byref(v), None)
        return bool(v.value & 0x100)

    def set_debug_option(self, option, value):
        """hikari_hip_debug.h hk_debug_set_option (F.DEBUG_OPT_*): the switches of tests and A/B tools - the library reads no environment variable."""
        self.api.call("debug_set_option", self.ctx, option, int(value))

    def main_stream_priority(self):
        """(high, decided): whether the context's own main stream was created at the device's highest priority, and whether the rule has
        decided yet - it does at the context's first frame (hikari_hip_debug.h hk_debug_main_stream_priority)."""
        v = F.u32()
        self.api.call("debug_main_stream_priority", self.ctx, C.byref(v))
        return bool(v.value & 1), bool(v.value & 2)

    def prepasses_pipelined(self):
        """frames whose primary rays ran on their own stream beside the previous frame's spatial pass (hk_debug_main_stream_priority, bits 8..27)"""
        v = F.u32()
        self.api.call("debug_main_stream_priority", self.ctx, C.byref(v))
        return int(v.value >> 8)

    def empty_tiles(self):
        """hk_debug_empty_tiles: (the empty-tile plane of the current frame parity as a (tiles_y, tiles_x) uint8 array, launches handed a plane so far)."""
        w, h, _ = self.buffer_info(F.BUF_TONE_MAPPED)
        tiles = np.zeros(((h + 7) // 8, (w + 7) // 8), dtype=np.uint8)
        n = C.c_uint64()
        self.api.call("debug_empty_tiles", self.ctx, tiles.ctypes.data_as(C.POINTER(C.c_uint8)), tiles.size, C.byref(n))
        return tiles, int(n.value)

    def spatial_windowed_launches(self):
        """spatial_reuse launches that took the windowed form of the kernel (hikari_hip_debug.h; F.DEBUG_OPT_SPATIAL_WINDOW)."""
        n = C.c_uint64()
        self.api.call("debug_spatial_windowed_launches", self.ctx, C.byref(n))
        return int(n.value)

    def spatial_known_launches(self):
        """spatial_reuse launches that were handed the table of the background's known records (hikari_hip_debug.h; F.DEBUG_OPT_SPATIAL_KNOWN)."""
        n = C.c_uint64()
        self.api.call("debug_spatial_known_launches", self.ctx, C.byref(n))
        return int(n.value)

    def measure_hbm(self, bytes_per_array=1 << 30, reps=8):
        """Empirical HBM ceiling: (copy GB/s, triad GB/s) of grid-stride float4 streams over arrays too big for the Infinity Cache."""
        cp, tr = C.c_double(), C.c_double()
        self.api.call("measure_hbm", self.ctx, bytes_per_array, reps, C.byref(cp), C.byref(tr))
        return cp.value, tr.value

    def measure_gather(self, footprint_bytes, bytes_per_step=32, waves_per_simd=7, steps=512, workgroups=0):
        """hk_measure_gather: (G wave-level loads / s, GB/s) of dependent divergent gathers over `footprint_bytes` of records."""
        a, b = C.c_double(), C.c_double()
        self.api.call("measure_gather", self.ctx, int(footprint_bytes), bytes_per_step, waves_per_simd, steps, workgroups, C.byref(a), C.byref(b))
        return a.value, b.value

    def measure_valu(self, iters=2048):
        """VALU issue ceiling: {waves per SIMD: 1e9 wave64 instructions per second} for 1, 2, 4, 8 resident waves per SIMD."""
        r = (C.c_double * 4)()
        self.api.call("measure_valu", self.ctx, iters, r)
        return {1 << k: r[k] for k in range(4)}

    def debug_math(self, op, x, y=None):
        """hk_debug_math: one f32 per item (include/hikari_hip_debug.h)."""
        return debug_math_call(self.api, self.ctx, op, x, y)


def debug_math_call(api, ctx, op, x, y=None):
    """debug_math of `api` (the library's, or the oracle's with ctx None).  The op decides the layout, as in probes.hip: ops 16..19
    and 35..52 read 16 floats of x per item, ops 46..49 four of y, every other op one of each.  Returns one f32 per item."""
    op = int(op)
    x = np.ascontiguousarray(x, dtype=np.float32)
    width = 16 if 16 <= op <= 19 or 35 <= op <= 52 else 1
    n, rest = divmod(x.size, width)
    if rest:
        raise ValueError(f"debug_math op {op} reads {width} floats of x per item, got {x.size}")
    yy = None if y is None else np.ascontiguousarray(y, dtype=np.float32)
    ywidth = 4 if 46 <= op <= 49 else 1
    if ywidth == 4 and yy is None:
        raise ValueError(f"debug_math op {op} takes its vector in y")
    if yy is not None and yy.size != ywidth * n:
        raise ValueError(f"debug_math op {op} reads {ywidth} floats of y per item: {ywidth * n} for {n} items, got {yy.size}")
    out = np.empty(n, dtype=np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(F.f32))
    api.call("debug_math", ctx, op, fp(x), None if yy is None else fp(yy), fp(out), n)
    return out


# ---------------------------------------------------------------------------------------------
# the reference's nodes and plugin
# ---------------------------------------------------------------------------------------------
class FrameCounter:  # view.rs:75-103: inserted as 0 on a new camera, +1 every frame
    def __init__(self, value=0):
        self.value = value

    def tick(self):
        self.value += 1
        return self.value


def frame_uniform(settings: HikariSettings, frame_number: int):
    """FrameUniform::extract_component (view.rs:141-193), evaluated by the library."""
    f = F.HkFrame()
    s = settings.to_c()
    F.api().call("frame_from_settings", C.byref(s), frame_number, C.byref(f))
    return f


class _Node:
    IN_VIEW = "view"  # light.rs:572

    def __init__(self, engine: Engine):
        self.engine = engine


class PrepassNode(_Node):  # prepass.rs:736-852
    def run(self, settings: HikariSettings):
        self.engine.set_view_options(settings.taa, settings.upscale.kind, settings.upscale.sharpness_)
        self.engine.pass_run(F.PASS_PREPASS)


class LightNode(_Node):  # light.rs:557-703
    def run(self, settings: HikariSettings):
        e = self.engine
        e.pass_run(F.PASS_FULL_SCREEN_ALBEDO)                      # light.rs:646-653
        e.pass_run(F.PASS_DIRECT_LIT)                              # light.rs:656-688, render[0], reservoirs (0,4)
        e.pass_run(F.PASS_DIRECT_EMISSIVE)                         # render[1], reservoirs (2,4)
        if settings.emissive_spatial_reuse:                        # light.rs:675,689-697
            e.pass_run(F.PASS_EMISSIVE_SPATIAL_REUSE)
        e.pass_run(F.PASS_INDIRECT)                                # render[2], reservoirs (6,8)
        if settings.indirect_spatial_reuse:                        # light.rs:676
            e.pass_run(F.PASS_INDIRECT_SPATIAL_REUSE)


class PostProcessNode(_Node):  # post_process.rs:1107-1312
    def run(self, settings: HikariSettings, antialias=False):
        e = self.engine
        if settings.denoise:                                       # post_process.rs:1190-1224
            channels = 2 if settings.indirect_bounces == 0 else 3  # post_process.rs:949-954
            for ch in range(channels):
                e.pass_run(F.PASS_DEMODULATION, ch)
                for level in range(4):
                    e.pass_run(F.PASS_DENOISE_L0 + level, ch)
        e.pass_run(F.PASS_TONE_MAPPING, int(settings.denoise))     # post_process.rs:1226-1234
        if antialias:
            self.run_antialias(settings)

    def run_antialias(self, settings: HikariSettings):
        e = self.engine
        e.set_view_options(settings.taa, settings.upscale.kind, settings.upscale.sharpness_)
        if settings.upscale.kind == F.UPSCALE_SMAA_TU4X:           # post_process.rs:1236-1258
            e.pass_run(F.PASS_SMAA_TU4X)
            e.pass_run(F.PASS_SMAA_TU4X_EXTRAPOLATE)
        if settings.taa == Taa.Jasmine:                            # post_process.rs:1260-1275
            e.pass_run(F.PASS_TAA_JASMINE)
        if settings.upscale.kind == F.UPSCALE_FSR1:                # post_process.rs:1277-1308
            e.pass_run(F.PASS_FSR_EASU)
            e.pass_run(F.PASS_FSR_RCAS)


class OverlayNode(_Node):  # overlay.rs:311-395
    def run(self, settings: HikariSettings, *, antialias, **kwargs):
        return self.engine.present(settings, antialias=antialias, **kwargs)


class HikariPlugin:
    """App::add_plugin(HikariPlugin): owns the context, uploads the noise tiles at start-up
    (lib.rs:189-219) and renders one camera with the `hikari` sub-graph order
    PREPASS -> LIGHT -> POST_PROCESS (lib.rs:252-367)."""

    def __init__(self, device=0, universal_settings: Optional[HikariUniversalSettings] = None, flags=0, api=None):
        self.universal_settings = universal_settings or HikariUniversalSettings()
        self.engine = Engine(api=api, device=device, flags=flags)
        self.engine.upload_noise()
        self.prepass, self.light, self.post_process = PrepassNode(self.engine), LightNode(self.engine), PostProcessNode(self.engine)
        self.overlay = OverlayNode(self.engine)
        self.counter = FrameCounter(0)
        self._size = None
        self._previous_camera = None

    def set_scene(self, scene: SceneData):
        self.engine.upload_scene(scene)

    def load_scene(self, builder, mode=F.TREE_SAH, textures=()):
        """set_scene for a finished SceneBuilder with deferred meshes: their trees are built on the device (Engine.load_scene)."""
        return self.engine.load_scene(builder, mode, textures)

    def add_meshes(self, builder, mode=F.TREE_SAH, sources=None, producer_stream=None):
        """Meshes added to the loaded builder since (glTF assets that arrive frame by frame): appended on the device (Engine.add_meshes);
        `sources`: the arrays of the meshes declared by their counts, as torch tensors on the device."""
        self.engine.add_meshes(builder, mode, sources, producer_stream)

    def remove_meshes(self, extents):
        """Meshes that left the builder (SceneBuilder.remove_mesh): the device scene is compacted (Engine.remove_meshes)."""
        self.engine.remove_meshes(extents)

    def change_instances(self, builder, mode=F.TREE_SAH):
        """Instances spawned, despawned or re-materialed on the builder, in any state of the scene: Engine.change_instances."""
        self.engine.change_instances(builder, mode)

    def deform_meshes(self, items, producer_stream=None):
        """Per frame, every deforming mesh of the scene in one call: Engine.deform_meshes."""
        self.engine.deform_meshes(items, producer_stream)

    def set_mesh_motion_vectors(self, mesh, enabled=True):
        """Per-vertex motion vectors for one deforming mesh, on or off: Engine.set_mesh_motion_vectors."""
        self.engine.set_mesh_motion_vectors(mesh, enabled)

    def set_instance_transforms(self, builder, models, ids=None, producer_stream=None, status=None):
        """Per frame, instance poses that live in device memory: Engine.set_instance_transforms."""
        self.engine.set_instance_transforms(builder, models, ids, producer_stream, status)

    def read_instance_transforms(self):
        """The poses the device holds (Engine.read_instance_transforms)."""
        return self.engine.read_instance_transforms()

    def update_textures(self, items, producer_stream=None):
        """Per frame, textures whose texels live in device memory, many per call: Engine.update_textures."""
        self.engine.update_textures(items, producer_stream)

    def read_texture(self, index):
        """The texels the device holds of one texture (Engine.read_texture)."""
        return self.engine.read_texture(index)

    def update_instances(self, scene: SceneData):
        """Instances moved (prepare_instances, instance.rs:352-437): rewrite the instance-level buffers only."""
        self.engine.upload_instances(scene)

    def render(self, camera: Camera, settings: HikariSettings, lights=None, frame_number=None, by_nodes=False, antialias=False):
        """One frame of the camera's render graph.  Returns the frame number used.  antialias=True also runs the
        SMAA Tu4x / TAA dispatches of PostProcessNode::run (the north-star frame ends at tone mapping)."""
        size = (camera.width, camera.height, settings.upscale.ratio())
        if size != self._size:  # prepare_light_textures, light.rs:342-363: reallocate + zero on size change
            self.engine.resize(*size)
            self._size = size
        n = self.counter.tick() if frame_number is None else frame_number
        frame = frame_uniform(settings, n)
        view = camera.view_uniform()
        pview = camera.previous_view_uniform(self._previous_camera)
        lights = lights or lights_uniform()
        if by_nodes:
            self.engine.frame_begin(frame, view, pview, lights)
            self.prepass.run(settings)
            self.light.run(settings)
            self.post_process.run(settings, antialias)
        else:
            self.engine.frame_render(frame, view, pview, lights, settings.to_c(), F.FRAME_ANTIALIAS if antialias else 0)
        self._previous_camera = camera
        return n

    def reset_history(self):
        """The next frame starts from an empty temporal history, as a new camera's first frame does: every screen buffer is reallocated and
        zeroed (a resize away and back, behind a wait for the frames in flight; prepare_light_textures, light.rs:342-363) and the previous
        camera is forgotten.  The scene stays."""
        self._previous_camera = None
        if self._size is None:   # (no frame yet: the first one allocates)
            return
        w, h, ratio = self._size
        self.engine.wait()
        self.engine.resize(w + 8, h + 8, ratio)
        self.engine.resize(w, h, ratio)

    def present(self, settings: HikariSettings, *, antialias, **kwargs):
        """OverlayNode::run: the frame last rendered into a view target in device memory (Engine.present)."""
        return self.overlay.run(settings, antialias=antialias, **kwargs)

    def final_image(self, settings: HikariSettings):
        """What OverlayNode samples (overlay.rs:226-231), as f32 [H][W][4]."""
        if settings.upscale.kind == F.UPSCALE_SMAA_TU4X:
            buf = F.BUF_TAA_OUTPUT if settings.taa == Taa.Jasmine else F.BUF_UPSCALE_OUTPUT
        else:                                                       # upscale_output[1]: EASU then RCAS
            buf = F.BUF_UPSCALE_SHARPENED
        return self.engine.read_f16(buf)

    def output(self, settings: HikariSettings):
        """The three radiance channels the tone-mapping pass sums (tone_mapping.wgsl:25-27), as f32 [3][H][W][4]."""
        base = F.BUF_DENOISE_RENDER0 if settings.denoise else F.BUF_RENDER0
        return np.stack([self.engine.read_f16(base + i) for i in range(3)])
