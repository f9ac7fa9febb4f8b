// gpu_canaliseur.cc -- tsd_amd::canaliseur_polyphase: ONE wideband complex stream into nb_canaux channel rows, on the polyphase
// channelizer of the C ABI (include/tsdgpu.h: tsdgpu_channelizer).  An extension: libtsd has only the opposite direction, as a
// one-shot function.  Channel c (centre c / nb_canaux of the input rate) is shifted to DC, filtered with the real prototype h
// and decimated by nb_canaux.
// step(x, y): x.rows() = n must be a whole number of nb_canaux-sample frames; y is resized to nb_canaux blocks of n / nb_canaux
// samples, channel after channel -- the layout filtre_rif_canaux::step and the other banks take; host or resident vectors.
#include "gpu_commun.hpp"
#include "tsd_amd/extensions.hpp"

namespace tsd_amd {

struct CanaliseurGpu : FiltreGen<cfloat> {
  tsdgpu_channelizer *h = nullptr;
  entier M;
  CanaliseurGpu(const Vecf &taps, entier nb_canaux) : M(nb_canaux)
  {
    if (nb_canaux < 1) échec("canaliseur_polyphase: nb_canaux >= 1 required ({})", (int) nb_canaux);
    if (taps.rows() <= 0) échec("canaliseur_polyphase: K > 0 required (K = {})", (int) taps.rows());
    if (tsdgpu_channelizer_create(&h, (int) nb_canaux, taps.data(), (int) taps.rows())) gpu_fail("canaliseur_polyphase");
  }
  ~CanaliseurGpu() { tsdgpu_channelizer_destroy(h); }
  void step(const Vecteur<cfloat> &x, Vecteur<cfloat> &y)
  {
    const entier n = x.rows();
    if (n % M != 0) échec("canaliseur_polyphase::step: {} samples are not a whole number of {}-sample frames", (int) n, (int) M);
    const int64_t F = n / M;
    if ((const void *) x.data() == (const void *) y.data() && n > 0) échec("canaliseur_polyphase::step: x and y are the same vector");
    sortie_variable(x, y, (long long) n, [&](cfloat *out) {
      int64_t got = 0;
      if (n > 0 && tsdgpu_channelizer_step(h, x.data(), n, out, F, F, &got, nullptr)) gpu_fail("canaliseur_polyphase::step");
    });
  }
};

sptr<FiltreGen<cfloat>> canaliseur_polyphase(const Vecf &h, entier nb_canaux) { return std::make_shared<CanaliseurGpu>(h, nb_canaux); }

}  // namespace tsd_amd
