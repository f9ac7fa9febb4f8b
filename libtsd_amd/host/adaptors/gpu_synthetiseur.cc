// gpu_synthetiseur.cc -- tsd_amd::synthetiseur_polyphase: nb_canaux channel rows into ONE wideband complex stream, on the polyphase
// synthesizer of the C ABI (include/tsdgpu.h: tsdgpu_synthesizer).  An extension: libtsd has this direction only as a one-shot
// function.  Channel c is upsampled by nb_canaux, filtered at baseband with the real prototype h, then shifted to c / nb_canaux
// of the output rate; the channels are summed.
// step(x, y): x.rows() = nb_canaux blocks of F samples, channel after channel -- what canaliseur_polyphase::step and the banks
// produce; y is resized to nb_canaux * F samples of the wideband stream; host or resident vectors.
#include "gpu_commun.hpp"
#include "tsd_amd/extensions.hpp"

namespace tsd_amd {

struct SynthetiseurGpu : FiltreGen<cfloat> {
  tsdgpu_synthesizer *h = nullptr;
  entier M;
  SynthetiseurGpu(const Vecf &taps, entier nb_canaux) : M(nb_canaux)
  {
    if (nb_canaux < 1) échec("synthetiseur_polyphase: nb_canaux >= 1 required ({})", (int) nb_canaux);
    if (taps.rows() <= 0) échec("synthetiseur_polyphase: K > 0 required (K = {})", (int) taps.rows());
    if (tsdgpu_synthesizer_create(&h, (int) nb_canaux, taps.data(), (int) taps.rows())) gpu_fail("synthetiseur_polyphase");
  }
  ~SynthetiseurGpu() { tsdgpu_synthesizer_destroy(h); }
  void step(const Vecteur<cfloat> &x, Vecteur<cfloat> &y)
  {
    const entier n = x.rows();
    if (n % M != 0) échec("synthetiseur_polyphase::step: {} samples are not {} blocks of one length", (int) n, (int) M);
    const int64_t F = n / M;
    if ((const void *) x.data() == (const void *) y.data() && n > 0) échec("synthetiseur_polyphase::step: x and y are the same vector");
    sortie_variable(x, y, (long long) n, [&](cfloat *out) {
      int64_t got = 0;
      if (n > 0 && tsdgpu_synthesizer_step(h, x.data(), F, F, out, n, &got, nullptr)) gpu_fail("synthetiseur_polyphase::step");
    });
  }
};

sptr<FiltreGen<cfloat>> synthetiseur_polyphase(const Vecf &h, entier nb_canaux) { return std::make_shared<SynthetiseurGpu>(h, nb_canaux); }

}  // namespace tsd_amd
