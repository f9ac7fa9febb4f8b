// gpu_synthetiseur.cc -- tsd_amd::synthetiseur_polyphase: nb_canaux channel rows into ONE wideband complex stream, on the polyphase
// synthesizer of the C ABI (include/tsdgpu.h: tsdgpu_synthesizer).  An extension: libtsd has this direction only as a one-shot
// function.  Channel c is upsampled by nb_canaux, filtered at baseband with the real prototype h, then shifted to c / nb_canaux
// of the output rate; the channels are summed.
// step(x, y): x.rows() = nb_canaux blocks of F samples, channel after channel -- what canaliseur_polyphase::step and the banks
// produce; y is resized to nb_canaux * F samples of the wideband stream; host or resident vectors.
// With surech = OS in {2, 4} (the three-argument factory) the bank is oversampled: a frame per hop of D = nb_canaux / OS output
// samples, y is resized to D * F samples.
#include "gpu_commun.hpp"
#include "tsd_amd/extensions.hpp"

namespace tsd_amd {

struct SynthetiseurGpu : FiltreGen<cfloat> {
  tsdgpu_synthesizer *h = nullptr;
  entier M, D;                          // channels, hop
  SynthetiseurGpu(const Vecf &taps, entier nb_canaux, entier surech) : M(nb_canaux), D(nb_canaux)
  {
    if (nb_canaux < 1) échec("synthetiseur_polyphase: nb_canaux >= 1 required ({})", (int) nb_canaux);
    if (surech < 1) échec("synthetiseur_polyphase: surech >= 1 required ({})", (int) surech);
    if (taps.rows() <= 0) échec("synthetiseur_polyphase: K > 0 required (K = {})", (int) taps.rows());
    const int rc = surech == 1 ? tsdgpu_synthesizer_create(&h, (int) nb_canaux, taps.data(), (int) taps.rows())
                               : tsdgpu_synthesizer_create_oversampled(&h, (int) nb_canaux, (int) surech, taps.data(), (int) taps.rows());
    if (rc) gpu_fail("synthetiseur_polyphase");
    D = tsdgpu_synthesizer_hop(h);
  }
  ~SynthetiseurGpu() { tsdgpu_synthesizer_destroy(h); }
  void step(const Vecteur<cfloat> &x, Vecteur<cfloat> &y)
  {
    const entier n = x.rows();
    if (n % M != 0) échec("synthetiseur_polyphase::step: {} samples are not {} blocks of one length", (int) n, (int) M);
    const int64_t F = n / M;
    if ((const void *) x.data() == (const void *) y.data() && n > 0) échec("synthetiseur_polyphase::step: x and y are the same vector");
    sortie_variable(x, y, (long long) D * F, [&](cfloat *out) {
      int64_t got = 0;
      if (n > 0 && tsdgpu_synthesizer_step(h, x.data(), F, F, out, D * F, &got, nullptr)) gpu_fail("synthetiseur_polyphase::step");
    });
  }
};

sptr<FiltreGen<cfloat>> synthetiseur_polyphase(const Vecf &h, entier nb_canaux) { return std::make_shared<SynthetiseurGpu>(h, nb_canaux, 1); }

sptr<FiltreGen<cfloat>> synthetiseur_polyphase(const Vecf &h, entier nb_canaux, entier surech)
{
  return std::make_shared<SynthetiseurGpu>(h, nb_canaux, surech);
}

}  // namespace tsd_amd
