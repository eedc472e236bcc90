// image_view_check.cpp -- the host's view of a packed model image (judo_amd/csrc/jh_image.h) and its readers on an image file, then on that image with every named
// count and offset overwritten and each section cut short.  Plain C++, no HIP and no library: tests/test_image_layout.py compiles it with the address and
// undefined-behaviour sanitizers and compares what it prints with judo_amd/engine_model.py::image_offsets.
//   usage: image_view_check IMAGE      prints "name value" lines; exit 0 unless the file cannot be read (a sanitizer report ends the run with its own status)
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "jh_image.h"

static char g_err[512] = "";
void jh_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

using namespace jh_eng;

// What jh_model_create asks of an image of `kind` (2: the leap family, 3: fr3_pick): true if the view does not fit or a reader calls the image malformed.
// An image that passes has every reader run over it, and pair_tables_shared against itself.
static bool refused(int kind, const std::vector<float>& F, const std::vector<int>& I) {
  HostImage im;
  im.bind(F.data(), I.data(), F.size(), I.size());
  if (image_cylinders(im) < 0) return true;
  if (kind == 2 && image_pair_tables(im) < 0) return true;
  if (kind == 3 && image_arm_pairs(im) < 0) return true;
  (void)pair_tables_shared(im, im);
  return !im.fits;
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s IMAGE\n", argv[0]); return 2; }
  FILE* fp = fopen(argv[1], "rb");
  uint32_t h[16];
  if (!fp || fread(h, 4, 16, fp) != 16) { fprintf(stderr, "%s: no blob header\n", argv[1]); return 2; }
  const int kind = (int)h[2];
  std::vector<float> F(h[8]);  // (exactly the sections' sizes on the heap: a read past either end is a sanitizer report)
  std::vector<int> I(h[9]);
  if (fread(F.data(), 4, F.size(), fp) != F.size() || fread(I.data(), 4, I.size(), fp) != I.size()) { fprintf(stderr, "%s: short sections\n", argv[1]); return 2; }
  fclose(fp);

  HostImage im;
  im.bind(F.data(), I.data(), F.size(), I.size());
  const EngineModel& v = im.v;
  printf("fits %d\n", (int)im.fits);
  if (!im.fits) return 0;
#define P(name, value) printf(#name " %d\n", (int)(value))
#define PV(name) P(name, v.name)
#define PI(name) P(name, im.name)
  PV(NM); PV(NBLK); PV(NV); PV(NQ); PV(NU); PV(NG); PV(NSITE); PV(NS); PV(NSENS); PV(cone);
  PV(oBodyI); PV(oBlockI); PV(oActI); PV(oGeomI); PV(oSiteI); PV(oSensI); PV(oBodyF); PV(oDofF); PV(oActF); PV(oGeomF); PV(oSiteF);
  PV(NAG); PV(NPAIR); PV(NEQ); PV(NFRAME); PV(NDIST); PV(NGS);
  PV(oAGI); PV(oPairI); PV(oEqI); PV(oFrameI); PV(oDistI); PV(oSensG); PV(oGlist); PV(oAGF); PV(oGPF); PV(oEqF); PV(oFrameF); PV(oDistF);
  PI(oLane); PI(LGM); PI(oBP); PI(NBP); PI(oBG); PI(oBS); PI(oRef); PI(oPT);
  P(cylinders, image_cylinders(im));
  P(arm_pairs, image_arm_pairs(im));
  P(pair_tables, image_pair_tables(im));
  P(shared_with_itself, pair_tables_shared(im, im));

  // every named count and offset, in the header and in the generic block, set to -1, nint, nfloat and 0x7fffffff in turn
  std::vector<int> slots = {HI_NM, HI_NBLK, HI_NV, HI_NQ, HI_NU, HI_NG, HI_NSITE, HI_NS, HI_NSENS, HI_LANES, HI_LGM, HI_GI, HI_GF, HI_BP, HI_BS, HI_NBP, HI_REF, HI_PT};
  for (int k : {GI_NAG, GI_NPAIR, GI_NEQ, GI_NFRAME, GI_NDIST, GI_NGS}) slots.push_back(I[HI_GI] + k);
  const int values[4] = {-1, (int)I.size(), (int)F.size(), 0x7fffffff};
  int mutations = 0, undetected = 0;
  for (int at : slots)
    for (int value : values) {
      std::vector<int> J = I;
      J[at] = value;
      mutations++;
      if (!refused(kind, F, J)) { undetected++; printf("undetected %d %d\n", at, value); }
    }
  {  // each section one word short
    const std::vector<int> J(I.begin(), I.end() - 1);
    const std::vector<float> E(F.begin(), F.end() - 1);
    mutations += 2;
    if (!refused(kind, F, J)) { undetected++; printf("undetected int_section_short 0\n"); }
    if (!refused(kind, E, I)) { undetected++; printf("undetected float_section_short 0\n"); }
  }
  P(mutations, mutations);
  P(undetected_mutations, undetected);
  return 0;
}
