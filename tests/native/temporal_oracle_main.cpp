// A stand-alone host program over oracle/hk_oracle.cpp alone, meant to be built with -fsanitize=address,undefined
// (tests/test_temporal_planes.py does so): it replays dispatches of the temporal light passes from the flat files that
// post_planes.dump_temporal_planes writes - one file per argument - through the oracle's C entry points.  The `edge` planes put a
// previous_uv of exactly 1 on the last row, which forms a slot one row past previous_spatial: an oracle that queues, parks or applies
// that store reads and writes beyond its buffers, and the sanitizer says so.  Exit status 0 and "ok" on success.
//
// The file: a sequence of blobs, each a u64 byte count and the bytes - a header (window width, height, the ratio as f32, the pass id,
// the number of buffers), vertices, primitives, mesh nodes, materials, instances, instance nodes, emissives, emissive nodes, the alias
// table, the noise tiles, HkFrame, HkView, HkPreviousView, HkLights, then per buffer its id (u32) and its contents.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "hikari_hip.h"

struct orc_ctx;
extern "C" {
const char* orc_last_error(void);
int orc_create(int device_id, uint32_t flags, orc_ctx** out);
void orc_destroy(orc_ctx* ctx);
int orc_set_threads(int n);
int orc_upload_meshes(orc_ctx* ctx, const HkVertex* v, uint32_t nv, const HkPrimitive* p, uint32_t np, const HkNode* n, uint32_t nn);
int orc_upload_materials(orc_ctx* ctx, const HkMaterial* m, uint32_t n);
int orc_upload_instances(orc_ctx* ctx, const HkInstance* inst, uint32_t ni, const HkNode* inodes, uint32_t nin, const HkEmissive* em, uint32_t ne,
                         const HkNode* enodes, uint32_t nen, const HkAliasEntry* alias, uint32_t na);
int orc_upload_noise(orc_ctx* ctx, const uint8_t* rgba, size_t bytes);
int orc_resize(orc_ctx* ctx, uint32_t width, uint32_t height, float upscale_ratio);
int orc_frame_begin(orc_ctx* ctx, const HkFrame* f, const HkView* v, const HkPreviousView* pv, const HkLights* l);
int orc_pass_run(orc_ctx* ctx, uint32_t pass, uint32_t arg, uint32_t row_begin, uint32_t row_end);
int orc_write_buffer(orc_ctx* ctx, uint32_t buffer, const void* src, size_t bytes);
int orc_read_buffer(orc_ctx* ctx, uint32_t buffer, void* dst, size_t bytes);
}

#define CHECK(cond)                                                                       \
  do {                                                                                    \
    if (!(cond)) {                                                                        \
      fprintf(stderr, "%s:%d: %s failed: %s\n", __FILE__, __LINE__, #cond, orc_last_error()); \
      return 1;                                                                           \
    }                                                                                     \
  } while (0)

typedef std::vector<uint8_t> Blob;   // (copied to exactly its size on the heap: a read past a blob's end is a sanitizer report too)

static bool read_blob(FILE* f, Blob* out) {
  uint64_t n = 0;
  if (fread(&n, sizeof n, 1, f) != 1 || n > (1ull << 30)) return false;
  out->resize((size_t)n);
  return n == 0 || fread(out->data(), 1, (size_t)n, f) == (size_t)n;
}
template <class T>
static uint32_t count_of(const Blob& b) { return (uint32_t)(b.size() / sizeof(T)); }
template <class T>
static const T* as(const Blob& b) { return b.empty() ? nullptr : reinterpret_cast<const T*>(b.data()); }

static int replay(const char* path) {
  FILE* f = fopen(path, "rb");
  CHECK(f);
  Blob header, scene[9], noise, frame, view, pview, lights;
  CHECK(read_blob(f, &header) && header.size() == 20);
  for (Blob& b : scene) CHECK(read_blob(f, &b));
  CHECK(read_blob(f, &noise) && read_blob(f, &frame) && read_blob(f, &view) && read_blob(f, &pview) && read_blob(f, &lights));
  CHECK(frame.size() == sizeof(HkFrame) && view.size() == sizeof(HkView) && pview.size() == sizeof(HkPreviousView) && lights.size() == sizeof(HkLights));
  uint32_t width, height, pass, n_buffers;
  float ratio;
  memcpy(&width, header.data(), 4); memcpy(&height, header.data() + 4, 4); memcpy(&ratio, header.data() + 8, 4);
  memcpy(&pass, header.data() + 12, 4); memcpy(&n_buffers, header.data() + 16, 4);

  orc_ctx* c = nullptr;
  CHECK(orc_create(0, 0, &c) == HK_OK);
  CHECK(orc_upload_meshes(c, as<HkVertex>(scene[0]), count_of<HkVertex>(scene[0]), as<HkPrimitive>(scene[1]), count_of<HkPrimitive>(scene[1]),
                          as<HkNode>(scene[2]), count_of<HkNode>(scene[2])) == HK_OK);
  CHECK(orc_upload_materials(c, as<HkMaterial>(scene[3]), count_of<HkMaterial>(scene[3])) == HK_OK);
  CHECK(orc_upload_instances(c, as<HkInstance>(scene[4]), count_of<HkInstance>(scene[4]), as<HkNode>(scene[5]), count_of<HkNode>(scene[5]),
                             as<HkEmissive>(scene[6]), count_of<HkEmissive>(scene[6]), as<HkNode>(scene[7]), count_of<HkNode>(scene[7]),
                             as<HkAliasEntry>(scene[8]), count_of<HkAliasEntry>(scene[8])) == HK_OK);
  CHECK(orc_upload_noise(c, noise.data(), noise.size()) == HK_OK);
  CHECK(orc_resize(c, width, height, ratio) == HK_OK);
  CHECK(orc_frame_begin(c, as<HkFrame>(frame), as<HkView>(view), as<HkPreviousView>(pview), as<HkLights>(lights)) == HK_OK);
  std::vector<uint32_t> ids;
  std::vector<size_t> sizes;
  for (uint32_t i = 0; i < n_buffers; ++i) {
    Blob id, data;
    CHECK(read_blob(f, &id) && id.size() == 4 && read_blob(f, &data));
    uint32_t buffer;
    memcpy(&buffer, id.data(), 4);
    CHECK(orc_write_buffer(c, buffer, data.data(), data.size()) == HK_OK);
    ids.push_back(buffer);
    sizes.push_back(data.size());
  }
  fclose(f);
  CHECK(orc_pass_run(c, pass, 0, 0, 0) == HK_OK);
  uint64_t sum = 0;   // (every buffer read back whole: what the pass wrote is touched once more, inside its bounds)
  for (size_t i = 0; i < ids.size(); ++i) {
    Blob back(sizes[i]);
    CHECK(orc_read_buffer(c, ids[i], back.data(), back.size()) == HK_OK);
    for (uint8_t v : back) sum += v;
  }
  orc_destroy(c);
  printf("%s: pass %u, %u x %u at %.2f, checksum %llu\n", path, pass, width, height, (double)ratio, (unsigned long long)sum);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s planes.bin [planes.bin ...]\n", argv[0]);
    return 2;
  }
  orc_set_threads(1);   // (one thread: a report names one stack, and the run does not depend on the machine's core count)
  for (int i = 1; i < argc; ++i)
    if (int rc = replay(argv[i])) return rc;
  printf("ok\n");
  return 0;
}
