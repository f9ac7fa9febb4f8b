// gpu_canaux_rythme.cc -- tsd_amd::filtre_rif_decim_canaux / filtre_rif_demi_bande_canaux / filtre_rif_ups_canaux /
// decimateur_canaux: C channels through ONE integer-rate stage in one object, on the rate-changing channel bank of the C ABI
// (include/tsdgpu.h: tsdgpu_polyfir_bank).  An extension, like gpu_canaux.cc: each channel behaves as its own filtre_rif_decim
// / filtre_rif_demi_bande / filtre_rif_ups / decimateur object fed the same blocks.
// step(x, y): x holds nb_canaux blocks of n samples one after the other, y is resized to nb_canaux blocks of n_out samples in
// the same layout (every channel produces the same n_out); host or resident vectors, x and y may be the same object.
#include "gpu_commun.hpp"
#include "tsd_amd/extensions.hpp"

namespace tsd_amd {

template <typename T> struct EtageCanauxGpu : FiltreGen<T> {
  tsdgpu_polyfir_bank *h = nullptr;
  entier C;
  const char *qui;
  EtageCanauxGpu(const char *nom, int kind, const float *taps, entier K, entier R, entier nb_canaux) : C(nb_canaux), qui(nom)
  {
    if (nb_canaux < 1) échec("{}: nb_canaux >= 1 required ({})", qui, (int) nb_canaux);
    if (kind != TSDGPU_POLY_PICK && K <= 0) échec("{}: K > 0 required (K = {})", qui, (int) K);
    if (tsdgpu_polyfir_bank_create(&h, kind, dtype_of<T>(), taps, (int) K, (int) R, (int) nb_canaux)) gpu_fail(qui);
  }
  ~EtageCanauxGpu() { tsdgpu_polyfir_bank_destroy(h); }
  void step(const Vecteur<T> &x, Vecteur<T> &y)
  {
    const entier N = x.rows();
    if (N % C != 0) échec("{}::step: {} samples are not {} channels of the same length", qui, (int) N, (int) C);
    const entier n = N / C;
    const int64_t cap = tsdgpu_polyfir_bank_out_count(h, n);
    sortie_variable(x, y, cap * C, [&](T *out) {
      int64_t got = 0;
      if (n > 0 && tsdgpu_polyfir_bank_step(h, x.data(), n, n, out, cap, cap, &got, nullptr)) gpu_fail(qui);
    });
  }
};

template <typename Tc, typename T> sptr<FiltreGen<T>> filtre_rif_decim_canaux(const Vecteur<Tc> &c, entier R, entier nb_canaux)
{
  return std::make_shared<EtageCanauxGpu<T>>("filtre_rif_decim_canaux", TSDGPU_POLY_DECIM, c.data(), c.rows(), R, nb_canaux);
}
template <typename Tc, typename T> sptr<FiltreGen<T>> filtre_rif_demi_bande_canaux(const Vecteur<Tc> &c, entier nb_canaux)
{
  return std::make_shared<EtageCanauxGpu<T>>("filtre_rif_demi_bande_canaux", TSDGPU_POLY_HALFBAND, c.data(), c.rows(), 2, nb_canaux);
}
template <typename Tc, typename T> sptr<FiltreGen<T>> filtre_rif_ups_canaux(const Vecteur<Tc> &c, entier R, entier nb_canaux)
{
  return std::make_shared<EtageCanauxGpu<T>>("filtre_rif_ups_canaux", TSDGPU_POLY_UPS, c.data(), c.rows(), R, nb_canaux);
}
template <typename T> sptr<FiltreGen<T>> decimateur_canaux(entier R, entier nb_canaux)
{
  return std::make_shared<EtageCanauxGpu<T>>("decimateur_canaux", TSDGPU_POLY_PICK, nullptr, 0, R, nb_canaux);
}
template sptr<FiltreGen<float>> filtre_rif_decim_canaux<float, float>(const Vecteur<float> &, entier, entier);
template sptr<FiltreGen<cfloat>> filtre_rif_decim_canaux<float, cfloat>(const Vecteur<float> &, entier, entier);
template sptr<FiltreGen<float>> filtre_rif_demi_bande_canaux<float, float>(const Vecteur<float> &, entier);
template sptr<FiltreGen<cfloat>> filtre_rif_demi_bande_canaux<float, cfloat>(const Vecteur<float> &, entier);
template sptr<FiltreGen<float>> filtre_rif_ups_canaux<float, float>(const Vecteur<float> &, entier, entier);
template sptr<FiltreGen<cfloat>> filtre_rif_ups_canaux<float, cfloat>(const Vecteur<float> &, entier, entier);
template sptr<FiltreGen<float>> decimateur_canaux<float>(entier, entier);
template sptr<FiltreGen<cfloat>> decimateur_canaux<cfloat>(entier, entier);

}  // namespace tsd_amd
