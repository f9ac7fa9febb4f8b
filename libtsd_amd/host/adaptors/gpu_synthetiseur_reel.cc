// gpu_synthetiseur_reel.cc -- tsd_amd::synthetiseur_polyphase_reel: nb_canaux / 2 + 1 channel rows into ONE wideband REAL stream, on
// the real-output polyphase synthesizer of the C ABI (include/tsdgpu.h: tsdgpu_synthesizer_create_real).  An extension, like
// synthetiseur_polyphase (gpu_synthetiseur.cc), whose output on the block extended by the conjugate rows this is; the imaginary
// parts of rows 0 and nb_canaux / 2 are not used.
// step(x, y): x.rows() = nb_canaux / 2 + 1 blocks of F samples, channel after channel -- what canaliseur_polyphase_reel::step and the
// banks produce; y is resized to nb_canaux * F floats of the wideband stream; host or resident vectors.
#include "gpu_commun.hpp"
#include "tsd_amd/extensions.hpp"

namespace tsd_amd {

struct SynthetiseurReelGpu : FiltreGen<cfloat, float> {
  tsdgpu_synthesizer *h = nullptr;
  entier M, C;                          // frame length, rows
  SynthetiseurReelGpu(const Vecf &taps, entier nb_canaux) : M(nb_canaux), C(nb_canaux / 2 + 1)
  {
    if (nb_canaux < 1) échec("synthetiseur_polyphase_reel: nb_canaux >= 1 required ({})", (int) nb_canaux);
    if (taps.rows() <= 0) échec("synthetiseur_polyphase_reel: K > 0 required (K = {})", (int) taps.rows());
    if (tsdgpu_synthesizer_create_real(&h, (int) nb_canaux, 1, taps.data(), (int) taps.rows())) gpu_fail("synthetiseur_polyphase_reel");
    C = tsdgpu_synthesizer_rows(h);
  }
  ~SynthetiseurReelGpu() { tsdgpu_synthesizer_destroy(h); }
  void step(const Vecteur<cfloat> &x, Vecteur<float> &y)
  {
    const entier n = x.rows();
    if (n % C != 0) échec("synthetiseur_polyphase_reel::step: {} samples are not {} blocks of one length", (int) n, (int) C);
    const int64_t F = n / C;
    if ((const void *) x.data() == (const void *) y.data() && n > 0) échec("synthetiseur_polyphase_reel::step: x and y share their memory");
    sortie_variable(x, y, (long long) M * F, [&](float *out) {
      int64_t got = 0;
      if (n > 0 && tsdgpu_synthesizer_step(h, x.data(), F, F, out, M * F, &got, nullptr)) gpu_fail("synthetiseur_polyphase_reel::step");
    });
  }
};

sptr<FiltreGen<cfloat, float>> synthetiseur_polyphase_reel(const Vecf &h, entier nb_canaux)
{
  return std::make_shared<SynthetiseurReelGpu>(h, nb_canaux);
}

}  // namespace tsd_amd
