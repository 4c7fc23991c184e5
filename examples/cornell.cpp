// examples/cornell.cpp - the C++ twin of the reference's examples/cornell.rs (setup(): spawn
// models/cornell.glb, camera at (0,1,4) looking at (0,1,0), HikariSettings::default()), driving
// libhikari_hip.so through the C++ host mirror include/hikari.hpp.  Headless: renders N frames and
// writes the tone-mapped image as a PPM and/or the raw rgba16f words.  --present writes what the overlay hands the view target instead:
// the frame presented (hk_present) into a bgra8-sRGB image in device memory, as bytes.
//
//   cornell [--size W H] [--frames N] [--bounces B] [--ratio R | --fsr R SHARPNESS] [--by-nodes] [--antialias] [--ppm out.ppm] [--raw out.bin] [--describe]
//           [--present out.bgra]            OverlayNode: the last frame presented over its clear colour into a bgra8-sRGB target (W x H x 4 bytes)
//           [--pick U V]                    a ray query (hk_cast_rays) through the point (U, V) of the camera's image, 0..1 from its top left corner:
//                                          prints `pick instance primitive distance` (4294967295 4294967295 3.40282347e+38 for a miss); the frames are
//                                          the same with or without it
//           [--device-trees]                the meshes are added without their trees (SceneBuilder::add_mesh_deferred) and the scene is loaded with
//                                          load_scene: every mesh tree is built on the device (hk_load_scene); the frames are the same
//           [--animate [--rebuild-at F]]   the boxes drift every frame; the poses go to the GPU, which redoes the instance records and refits
//                                          both trees (hk_refit_scene_instances); at frame F the trees are rebuilt on the device (LBVH)
//           [--gpus N [--devices a,b,..]]   band-sharded over N GPUs from this one process (hk_multi_*); --devices may repeat an id
//           [--balance]                     ... with the bands split by cost on the first frame (HK_FRAME_BALANCE_BANDS)
//           [--gather]                      ... band 0's device collects the finished image every frame (HK_FRAME_GATHER)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>  // --present: the view target is device memory the HOST owns (hipMalloc / hipMemcpy / hipFree)

#include "hikari.hpp"

using namespace hikari;

static std::vector<uint8_t> read_file(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) throw std::runtime_error("cannot open " + path);
  return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

// assets/cornell.hkscene (tools/make_fixtures.py: make_cornell_bin) -> builder
static void load_cornell(const std::string& path, SceneBuilder& b, bool deferred = false) {
  std::vector<uint8_t> d = read_file(path);
  size_t off = 0;
  auto u32 = [&]() { uint32_t v; std::memcpy(&v, d.data() + off, 4); off += 4; return v; };
  auto floats = [&](size_t n) { std::vector<float> v(n); std::memcpy(v.data(), d.data() + off, n * 4); off += n * 4; return v; };
  if (std::memcmp(d.data(), "HKSC", 4) != 0) throw std::runtime_error("not an HKSC file");
  off = 4;
  uint32_t version = u32(), n_meshes = u32(), n_materials = u32(), n_instances = u32();
  if (version != 1) throw std::runtime_error("unsupported HKSC version");
  struct MeshData { std::vector<float> p, n, uv; std::vector<uint32_t> idx; uint32_t material; };
  std::vector<MeshData> meshes(n_meshes);
  for (auto& m : meshes) {
    uint32_t nv = u32(), ni = u32();
    m.material = u32();
    m.p = floats(nv * 3);
    m.n = floats(nv * 3);
    m.uv = floats(nv * 2);
    m.idx.resize(ni);
    std::memcpy(m.idx.data(), d.data() + off, ni * 4);
    off += ni * 4;
  }
  std::vector<uint32_t> material_ids;
  for (uint32_t i = 0; i < n_materials; ++i) {
    std::vector<float> v = floats(9);  // base_color[4], emissive[3], roughness, metallic
    material_ids.push_back(b.add_material(standard_material(&v[0], &v[4], v[7], v[8])));
  }
  std::vector<uint32_t> mesh_ids;
  for (auto& m : meshes) mesh_ids.push_back(deferred ? b.add_mesh_deferred(m.p, m.n, m.uv, m.idx) : b.add_mesh(m.p, m.n, m.uv, m.idx));
  for (uint32_t i = 0; i < n_instances; ++i) {
    uint32_t mesh = u32();
    std::vector<float> t = floats(16);
    b.add_instance(mesh_ids[mesh], material_ids[meshes[mesh].material], t.data());
  }
  b.finish();
}

static float half_to_float(uint16_t h) {
  uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 0x1fu, m = h & 0x3ffu, u;
  if (e == 0) {
    float v = (float)m * 5.9604644775390625e-8f;
    return sign ? -v : v;
  }
  u = e == 31 ? (sign | 0x7f800000u | (m << 13)) : (sign | ((e + 112u) << 23) | (m << 13));
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

int main(int argc, char** argv) {
  uint32_t w = 256, h = 256;
  size_t frames = 8;
  HikariSettings settings;  // HikariSettings::default(), examples/cornell.rs:53
  bool by_nodes = false, describe = false, antialias = false, animate = false, device_trees = false;
  size_t rebuild_at = 0;
  uint32_t ctx_flags = 0;
  int gpus = 1;
  std::vector<int> devices;
  bool balance = false;  // --balance: split the bands by cost on the first frame (HK_FRAME_BALANCE_BANDS)
  bool pick = false;     // --pick U V: one closest-hit query through that point of the image
  double pick_u = 0.5, pick_v = 0.5;
  bool gather = false;   // --gather: band 0's device collects the finished image every frame (HK_FRAME_GATHER); --raw then reads that one context
  std::string ppm, raw, present, assets = "bevy-hikari_amd/assets";
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    if (a == "--size" && i + 2 < argc) { w = (uint32_t)atoi(argv[++i]); h = (uint32_t)atoi(argv[++i]); }
    else if (a == "--frames" && i + 1 < argc) frames = (size_t)atoi(argv[++i]);
    else if (a == "--bounces" && i + 1 < argc) settings.indirect_bounces = (size_t)atoi(argv[++i]);
    else if (a == "--ratio" && i + 1 < argc) settings.upscale = Upscale::SmaaTu4x((float)atof(argv[++i]));
    else if (a == "--fsr" && i + 2 < argc) { const float r = (float)atof(argv[++i]); settings.upscale = Upscale::Fsr1(r, (float)atof(argv[++i])); }  // ratio, sharpness
    else if (a == "--by-nodes") by_nodes = true;
    else if (a == "--antialias") antialias = true;  // SMAA Tu4x / TAA / FSR1 as the settings say; output = what the overlay presents
    else if (a == "--ppm" && i + 1 < argc) ppm = argv[++i];
    else if (a == "--raw" && i + 1 < argc) raw = argv[++i];
    else if (a == "--present" && i + 1 < argc) present = argv[++i];
    else if (a == "--pick" && i + 2 < argc) { pick = true; pick_u = atof(argv[++i]); pick_v = atof(argv[++i]); }
    else if (a == "--assets" && i + 1 < argc) assets = argv[++i];
    else if (a == "--describe") describe = true;
    else if (a == "--animate") animate = true;
    else if (a == "--device-trees") device_trees = true;
    else if (a == "--deterministic") ctx_flags |= HK_CTX_DETERMINISTIC_SCATTER;  // resolve the reference's scatter-store race reproducibly (motion)
    else if (a == "--rebuild-at" && i + 1 < argc) rebuild_at = (size_t)atoi(argv[++i]);
    else if (a == "--gpus" && i + 1 < argc) gpus = atoi(argv[++i]);
    else if (a == "--balance") balance = true;
    else if (a == "--gather") gather = true;
    else if (a == "--devices" && i + 1 < argc) {
      std::string list = argv[++i];
      for (size_t p = 0; p < list.size();) {
        size_t q = list.find(',', p);
        if (q == std::string::npos) q = list.size();
        devices.push_back(atoi(list.substr(p, q - p).c_str()));
        p = q + 1;
      }
    }
    else { std::fprintf(stderr, "unknown argument %s\n", a.c_str()); return 2; }
  }
  if (describe) {  // no GPU needed: host-side mirrors only
    HkSettings c = settings.to_c(), d;
    hk_settings_default(&d);
    std::printf("graph=%s nodes=%s,%s,%s,%s workgroup=%u noise=%u\n", graph::NAME, graph::node::PREPASS, graph::node::LIGHT, graph::node::POST_PROCESS,
                graph::node::OVERLAY, WORKGROUP_SIZE, NOISE_TEXTURE_COUNT);
    std::printf("defaults_match_library=%d ratio=%.1f abi=%u\n", std::memcmp(&c, &d, sizeof(c)) == 0, settings.upscale.ratio(), hk_abi_version());
    SceneBuilder b;
    load_cornell(assets + "/cornell.hkscene", b);
    const HkNode* nodes; uint32_t n_nodes; const HkEmissive* em; uint32_t n_em;
    check(hk_scene_builder_instance_nodes(b.handle(), &nodes, &n_nodes), "instance_nodes");
    check(hk_scene_builder_emissives(b.handle(), &em, &n_em), "emissives");
    std::printf("tlas_nodes=%u emissives=%u\n", n_nodes, n_em);
    return 0;
  }
  if (gpus > 1 || !devices.empty()) try {  // one process, several GPUs: the frame cut into one band per device
    if (devices.empty()) for (int d = 0; d < gpus; ++d) devices.push_back(d);
    HikariMultiGpuPlugin plugin(read_file(assets + "/noise_rgba8_16x64x64.bin"), devices);
    SceneBuilder scene;
    load_cornell(assets + "/cornell.hkscene", scene, device_trees);
    if (device_trees) plugin.load_scene(scene); else plugin.set_scene(scene);
    Camera camera = Camera::looking_at({0.0, 1.0, 4.0}, {0.0, 1.0, 0.0}, {0.0, 1.0, 0.0}, w, h);
    if (balance) plugin.balance_bands_on_next_frame();
    plugin.set_gather(gather);
    for (size_t n = 1; n <= frames; ++n) plugin.render(camera, settings, n, nullptr, antialias);
    plugin.wait();
    if (balance) {
      std::printf("band bounds:");
      for (uint32_t b : plugin.band_bounds((uint32_t)devices.size())) std::printf(" %u", b);
      std::printf("\n");
    }
    uint32_t rw = 0, rh = 0;
    std::vector<uint8_t> tm = gather ? plugin.read_gathered(HikariPlugin::final_buffer(settings, antialias), &rw, &rh)
                                     : plugin.read(HikariPlugin::final_buffer(settings, antialias), &rw, &rh);
    if (!raw.empty()) std::ofstream(raw, std::ios::binary).write((const char*)tm.data(), (std::streamsize)tm.size());
    std::printf("rendered %zu frames at %ux%u on %zu bands (output size %ux%u)\n", frames, w, h, devices.size(), rw, rh);
    return 0;
  } catch (const Error& e) {
    std::fprintf(stderr, "hikari error %d: %s\n", e.code, e.what());
    return e.code == HK_E_NO_DEVICE ? 3 : 1;
  }
  try {
    HikariPlugin plugin(read_file(assets + "/noise_rgba8_16x64x64.bin"), 0, ctx_flags);  // App::new().add_plugin(HikariPlugin)
    SceneBuilder scene;
    load_cornell(assets + "/cornell.hkscene", scene, device_trees);        // asset_server.load("models/cornell.glb#Scene0")
    if (device_trees) {
      plugin.load_scene(scene);
      if (scene.pending_mesh_trees() != 0u) { std::fprintf(stderr, "load_scene left %u mesh trees pending\n", scene.pending_mesh_trees()); return 1; }
    } else {
      plugin.set_scene(scene);
    }
    Camera camera = Camera::looking_at({0.0, 1.0, 4.0}, {0.0, 1.0, 0.0}, {0.0, 1.0, 0.0}, w, h);  // cornell.rs:49-50
    if (pick) {  // picking: what is under this point of the image (needs the scene only - no size, no frame)
      const HkRay ray = camera.ray_through(pick_u, pick_v);
      const HkRayHit hit = plugin.context().cast_rays(&ray, 1)[0];
      std::printf("pick %u %u %.9g\n", hit.instance, hit.primitive, hit.distance);
    }
    std::vector<HkInstance> rest;
    if (animate) {  // the poses the asset was loaded with
      const HkInstance* inst; uint32_t n_inst;
      check(hk_scene_builder_instances(scene.handle(), &inst, &n_inst), "hk_scene_builder_instances");
      rest.assign(inst, inst + n_inst);
    }
    for (size_t n = 1; n <= frames; ++n) {
      if (animate && n > 1) {  // a moving GlobalTransform -> InstanceEvent::Modified (instance.rs:137-176), served on the device
        for (uint32_t i : {6u, 7u}) {
          float m[16];
          std::memcpy(m, rest[i].model, sizeof(m));
          m[12] = rest[i].model[12] + 0.01f * (float)(n - 1) * (i == 6u ? 1.0f : -1.0f);
          scene.set_instance_transform(i, m);
        }
        const uint32_t moved = plugin.refit_instances(scene);
        if (moved != 2u) { std::fprintf(stderr, "refit moved %u instances, expected 2\n", moved); return 1; }
        if (n == rebuild_at) plugin.rebuild_trees();
      }
      plugin.render(camera, settings, n, by_nodes, nullptr, antialias);
    }
    plugin.wait();
    const uint32_t out_buffer = HikariPlugin::final_buffer(settings, antialias);
    std::vector<uint8_t> tm = plugin.context().read(out_buffer);
    uint32_t rw, rh, bpp;
    check(hk_buffer_info(plugin.context().get(), out_buffer, &rw, &rh, &bpp), "hk_buffer_info");
    if (!raw.empty()) std::ofstream(raw, std::ios::binary).write((const char*)tm.data(), (std::streamsize)tm.size());
    if (!ppm.empty()) {
      std::ofstream f(ppm, std::ios::binary);
      f << "P6\n" << rw << " " << rh << "\n255\n";
      const uint16_t* px = (const uint16_t*)tm.data();
      for (size_t i = 0; i < (size_t)rw * rh; ++i)
        for (int k = 0; k < 3; ++k) {
          float v = half_to_float(px[4 * i + k]);
          v = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
          f.put((char)(unsigned char)(std::pow(v, 1.0f / 2.2f) * 255.0f + 0.5f));
        }
    }
    if (!present.empty()) {  // OverlayNode::run into bevy's default view target format, cleared to the camera's clear colour
      HkPresentTarget t{};
      t.width = rw; t.height = rh; t.pitch_bytes = rw * 4u;
      t.format = HK_FORMAT_BGRA8_UNORM_SRGB;
      t.flags = HK_PRESENT_CLEAR;
      const HkSettings sc = settings.to_c();
      std::memcpy(t.clear, sc.clear_color, sizeof(t.clear));
      std::vector<uint8_t> bytes((size_t)rw * rh * 4u);
      if (hipMalloc(&t.ptr, bytes.size()) != hipSuccess) { std::fprintf(stderr, "hipMalloc failed\n"); return 1; }
      plugin.present(settings, antialias, t);
      plugin.wait();
      const hipError_t rc = hipMemcpy(bytes.data(), t.ptr, bytes.size(), hipMemcpyDeviceToHost);
      (void)hipFree(t.ptr);
      if (rc != hipSuccess) { std::fprintf(stderr, "hipMemcpy failed\n"); return 1; }
      std::ofstream(present, std::ios::binary).write((const char*)bytes.data(), (std::streamsize)bytes.size());
    }
    std::printf("rendered %zu frames at %ux%u (output size %ux%u)\n", frames, w, h, rw, rh);
  } catch (const Error& e) {
    std::fprintf(stderr, "hikari error %d: %s\n", e.code, e.what());
    return e.code == HK_E_NO_DEVICE ? 3 : 1;
  }
  return 0;
}
