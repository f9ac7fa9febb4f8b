// gpu_canaliseur.cc -- tsd_amd::canaliseur_polyphase: ONE wideband complex stream into nb_canaux channel rows, on the polyphase
// channelizer of the C ABI (include/tsdgpu.h: tsdgpu_channelizer).  An extension: libtsd has only the opposite direction, as a
// one-shot function.  Channel c (centre c / nb_canaux of the input rate) is shifted to DC, filtered with the real prototype h
// and decimated by nb_canaux.
// step(x, y): x.rows() = n must be a whole number of nb_canaux-sample frames; y is resized to nb_canaux blocks of n / nb_canaux
// samples, channel after channel -- the layout filtre_rif_canaux::step and the other banks take; host or resident vectors.
// With surech = OS in {2, 4} (the three-argument factory) the bank is oversampled: a frame every D = nb_canaux / OS samples,
// n a whole number of hops of D samples, y nb_canaux blocks of n / D samples.
#include "gpu_commun.hpp"
#include "tsd_amd/extensions.hpp"

namespace tsd_amd {

struct CanaliseurGpu : FiltreGen<cfloat> {
  tsdgpu_channelizer *h = nullptr;
  entier M, D;                          // channels, hop
  CanaliseurGpu(const Vecf &taps, entier nb_canaux, entier surech) : M(nb_canaux), D(nb_canaux)
  {
    if (nb_canaux < 1) échec("canaliseur_polyphase: nb_canaux >= 1 required ({})", (int) nb_canaux);
    if (surech < 1) échec("canaliseur_polyphase: surech >= 1 required ({})", (int) surech);
    if (taps.rows() <= 0) échec("canaliseur_polyphase: K > 0 required (K = {})", (int) taps.rows());
    const int rc = surech == 1 ? tsdgpu_channelizer_create(&h, (int) nb_canaux, taps.data(), (int) taps.rows())
                               : tsdgpu_channelizer_create_oversampled(&h, (int) nb_canaux, (int) surech, taps.data(), (int) taps.rows());
    if (rc) gpu_fail("canaliseur_polyphase");
    D = tsdgpu_channelizer_hop(h);
  }
  ~CanaliseurGpu() { tsdgpu_channelizer_destroy(h); }
  void step(const Vecteur<cfloat> &x, Vecteur<cfloat> &y)
  {
    const entier n = x.rows();
    if (n % D != 0) échec("canaliseur_polyphase::step: {} samples are not a whole number of {}-sample hops", (int) n, (int) D);
    const int64_t F = n / D;
    if ((const void *) x.data() == (const void *) y.data() && n > 0) échec("canaliseur_polyphase::step: x and y are the same vector");
    sortie_variable(x, y, (long long) M * F, [&](cfloat *out) {
      int64_t got = 0;
      if (n > 0 && tsdgpu_channelizer_step(h, x.data(), n, out, F, F, &got, nullptr)) gpu_fail("canaliseur_polyphase::step");
    });
  }
};

sptr<FiltreGen<cfloat>> canaliseur_polyphase(const Vecf &h, entier nb_canaux) { return std::make_shared<CanaliseurGpu>(h, nb_canaux, 1); }

sptr<FiltreGen<cfloat>> canaliseur_polyphase(const Vecf &h, entier nb_canaux, entier surech)
{
  return std::make_shared<CanaliseurGpu>(h, nb_canaux, surech);
}

}  // namespace tsd_amd
