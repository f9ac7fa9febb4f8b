// gpu_canaliseur_reel.cc -- tsd_amd::canaliseur_polyphase_reel: ONE wideband REAL stream into nb_canaux / 2 + 1 channel rows, on the
// real-input polyphase channelizer of the C ABI (include/tsdgpu.h: tsdgpu_channelizer_create_real).  An extension, like
// canaliseur_polyphase (gpu_canaliseur.cc), whose rows 0 .. nb_canaux / 2 on the widened stream these are; the other rows are their
// conjugates and are not produced.
// step(x, y): x.rows() = n floats must be a whole number of nb_canaux-sample frames; y is resized to nb_canaux / 2 + 1 blocks of
// n / nb_canaux samples, channel after channel -- the layout filtre_rif_canaux::step and the other banks take; host or resident vectors.
// With surech = OS in {2, 4} (the three-argument factory; tsdgpu_channelizer_create_real_oversampled) the bank is oversampled: a
// frame every D = nb_canaux / OS floats, n a whole number of hops of D floats, y nb_canaux / 2 + 1 blocks of n / D samples.
#include "gpu_commun.hpp"
#include "tsd_amd/extensions.hpp"

namespace tsd_amd {

struct CanaliseurReelGpu : FiltreGen<float, cfloat> {
  tsdgpu_channelizer *h = nullptr;
  entier M, C, D;                       // frame length, rows, hop
  CanaliseurReelGpu(const Vecf &taps, entier nb_canaux, entier surech) : M(nb_canaux), C(nb_canaux / 2 + 1), D(nb_canaux)
  {
    if (nb_canaux < 1) échec("canaliseur_polyphase_reel: nb_canaux >= 1 required ({})", (int) nb_canaux);
    if (surech < 1) échec("canaliseur_polyphase_reel: surech >= 1 required ({})", (int) surech);
    if (taps.rows() <= 0) échec("canaliseur_polyphase_reel: K > 0 required (K = {})", (int) taps.rows());
    const int rc = surech == 1 ? tsdgpu_channelizer_create_real(&h, (int) nb_canaux, 1, taps.data(), (int) taps.rows())
                               : tsdgpu_channelizer_create_real_oversampled(&h, (int) nb_canaux, (int) surech, taps.data(), (int) taps.rows());
    if (rc) gpu_fail("canaliseur_polyphase_reel");
    C = tsdgpu_channelizer_rows(h);
    D = tsdgpu_channelizer_hop(h);
  }
  ~CanaliseurReelGpu() { tsdgpu_channelizer_destroy(h); }
  void step(const Vecteur<float> &x, Vecteur<cfloat> &y)
  {
    const entier n = x.rows();
    if (n % D != 0)
      échec("canaliseur_polyphase_reel::step: {} samples are not a whole number of {}-sample {}", (int) n, (int) D, D == M ? "frames" : "hops");
    const int64_t F = n / D;
    if ((const void *) x.data() == (const void *) y.data() && n > 0) échec("canaliseur_polyphase_reel::step: x and y share their memory");
    sortie_variable(x, y, (long long) C * F, [&](cfloat *out) {
      int64_t got = 0;
      if (n > 0 && tsdgpu_channelizer_step(h, x.data(), n, out, F, F, &got, nullptr)) gpu_fail("canaliseur_polyphase_reel::step");
    });
  }
};

sptr<FiltreGen<float, cfloat>> canaliseur_polyphase_reel(const Vecf &h, entier nb_canaux)
{
  return std::make_shared<CanaliseurReelGpu>(h, nb_canaux, 1);
}

sptr<FiltreGen<float, cfloat>> canaliseur_polyphase_reel(const Vecf &h, entier nb_canaux, entier surech)
{
  return std::make_shared<CanaliseurReelGpu>(h, nb_canaux, surech);
}

}  // namespace tsd_amd
