// gpu_synthetiseur_reel.cc -- tsd_amd::synthetiseur_polyphase_reel: nb_canaux / 2 + 1 channel rows into ONE wideband REAL stream, on
// the real-output polyphase synthesizer of the C ABI (include/tsdgpu.h: tsdgpu_synthesizer_create_real).  An extension, like
// synthetiseur_polyphase (gpu_synthetiseur.cc), whose output on the block extended by the conjugate rows this is; the imaginary
// parts of rows 0 and nb_canaux / 2 are not used.
// step(x, y): x.rows() = nb_canaux / 2 + 1 blocks of F samples, channel after channel -- what canaliseur_polyphase_reel::step and the
// banks produce; y is resized to nb_canaux * F floats of the wideband stream; host or resident vectors.
// With surech = OS in {2, 4} (the three-argument factory; tsdgpu_synthesizer_create_real_oversampled) the bank is oversampled: a
// frame per hop of D = nb_canaux / OS floats, y resized to D * F floats.
#include "gpu_commun.hpp"
#include "tsd_amd/extensions.hpp"

namespace tsd_amd {

struct SynthetiseurReelGpu : FiltreGen<cfloat, float> {
  tsdgpu_synthesizer *h = nullptr;
  entier M, C, D;                       // frame length, rows, hop
  SynthetiseurReelGpu(const Vecf &taps, entier nb_canaux, entier surech) : M(nb_canaux), C(nb_canaux / 2 + 1), D(nb_canaux)
  {
    if (nb_canaux < 1) échec("synthetiseur_polyphase_reel: nb_canaux >= 1 required ({})", (int) nb_canaux);
    if (surech < 1) échec("synthetiseur_polyphase_reel: surech >= 1 required ({})", (int) surech);
    if (taps.rows() <= 0) échec("synthetiseur_polyphase_reel: K > 0 required (K = {})", (int) taps.rows());
    const int rc = surech == 1 ? tsdgpu_synthesizer_create_real(&h, (int) nb_canaux, 1, taps.data(), (int) taps.rows())
                               : tsdgpu_synthesizer_create_real_oversampled(&h, (int) nb_canaux, (int) surech, taps.data(), (int) taps.rows());
    if (rc) gpu_fail("synthetiseur_polyphase_reel");
    C = tsdgpu_synthesizer_rows(h);
    D = tsdgpu_synthesizer_hop(h);
  }
  ~SynthetiseurReelGpu() { tsdgpu_synthesizer_destroy(h); }
  void step(const Vecteur<cfloat> &x, Vecteur<float> &y)
  {
    const entier n = x.rows();
    if (n % C != 0) échec("synthetiseur_polyphase_reel::step: {} samples are not {} blocks of one length", (int) n, (int) C);
    const int64_t F = n / C;
    if ((const void *) x.data() == (const void *) y.data() && n > 0) échec("synthetiseur_polyphase_reel::step: x and y share their memory");
    sortie_variable(x, y, (long long) D * F, [&](float *out) {
      int64_t got = 0;
      if (n > 0 && tsdgpu_synthesizer_step(h, x.data(), F, F, out, D * F, &got, nullptr)) gpu_fail("synthetiseur_polyphase_reel::step");
    });
  }
};

sptr<FiltreGen<cfloat, float>> synthetiseur_polyphase_reel(const Vecf &h, entier nb_canaux)
{
  return std::make_shared<SynthetiseurReelGpu>(h, nb_canaux, 1);
}

sptr<FiltreGen<cfloat, float>> synthetiseur_polyphase_reel(const Vecf &h, entier nb_canaux, entier surech)
{
  return std::make_shared<SynthetiseurReelGpu>(h, nb_canaux, surech);
}

}  // namespace tsd_amd
