// gpu_canaux.cc -- tsd_amd::filtre_rif_canaux / filtre_sois_canaux: C channels of ONE filter in one object, on the channel
// banks of the C ABI (include/tsdgpu.h: tsdgpu_fir_bank, tsdgpu_sos_bank).  An extension: libtsd has no multichannel filter
// for these to stand in for; each channel behaves as its own filtre_rif / filtre_sois object fed the same blocks.
// step(x, y): x holds nb_canaux blocks of n samples one after the other (the storage of an n x nb_canaux Tab, so Tab::map of a
// libtsd matrix works), y the same layout; host or resident vectors, in place allowed.
#include "gpu_commun.hpp"
#include "tsd_amd/extensions.hpp"

namespace tsd_amd {

namespace {
template <typename V> entier bloc_canal(const V &x, entier nb_canaux, const char *qui)
{
  const entier N = x.rows();
  if (N % nb_canaux != 0) échec("{}: {} samples are not {} channels of the same length", qui, (int) N, (int) nb_canaux);
  return N / nb_canaux;
}
}  // namespace

template <typename T, typename Tc> struct FiltreRIFCanauxGpu : FiltreGen<T> {
  tsdgpu_fir_bank *h = nullptr;
  entier C;
  FiltreRIFCanauxGpu(const Vecteur<Tc> &c, entier nb_canaux, int méthode = TSDGPU_FIR_DIRECT) : C(nb_canaux)
  {
    if (c.rows() <= 0) échec("filtre_rif_canaux: K > 0 required (K = {})", (int) c.rows());
    if (nb_canaux < 1) échec("filtre_rif_canaux: nb_canaux >= 1 required ({})", (int) nb_canaux);
    if (tsdgpu_fir_bank_create_method(&h, dtype_of<T>(), dtype_of<Tc>(), c.data(), c.rows(), (int) nb_canaux, méthode))
      gpu_fail("filtre_rif_canaux");
  }
  ~FiltreRIFCanauxGpu() { tsdgpu_fir_bank_destroy(h); }
  void step(const Vecteur<T> &x, Vecteur<T> &y)
  {
    const entier n = bloc_canal(x, C, "filtre_rif_canaux::step");
    if (x.data() != y.data()) dimensionne(y, x.rows());
    if (n > 0 && tsdgpu_fir_bank_step(h, x.data(), n, y.data(), n, n, nullptr)) gpu_fail("filtre_rif_canaux::step");
  }
};

template <typename T> struct ChaineSOISCanauxGpu : FiltreGen<T> {
  tsdgpu_sos_bank *h = nullptr;
  entier C;
  ChaineSOISCanauxGpu(const FRat<cfloat> &f, entier nb_canaux, tsd::filtrage::RIIStructure structure) : C(nb_canaux)
  {
    if (nb_canaux < 1) échec("filtre_sois_canaux: nb_canaux >= 1 required ({})", (int) nb_canaux);
    const SectionsSOIS s = sections_sois(f);
    if (tsdgpu_sos_bank_create(&h, dtype_of<T>(), s.coefs.data(), (int) (s.coefs.size() / 5), s.gain, s.rii1.empty() ? nullptr : s.rii1.data(),
                               structure == tsd::filtrage::FormeDirecte2 ? 2 : 1, (int) nb_canaux))
      gpu_fail("filtre_sois_canaux");
  }
  ~ChaineSOISCanauxGpu() { tsdgpu_sos_bank_destroy(h); }
  void step(const Vecteur<T> &x, Vecteur<T> &y)
  {
    const entier n = bloc_canal(x, C, "filtre_sois_canaux::step");
    if (x.data() != y.data()) dimensionne(y, x.rows());
    if (n > 0 && tsdgpu_sos_bank_step(h, x.data(), n, y.data(), n, n, nullptr)) gpu_fail("filtre_sois_canaux::step");
  }
};

template <typename Tc, typename T> sptr<FiltreGen<T>> filtre_rif_canaux(const Vecteur<Tc> &h, entier nb_canaux)
{
  return std::make_shared<FiltreRIFCanauxGpu<T, Tc>>(h, nb_canaux);
}
template sptr<FiltreGen<float>> filtre_rif_canaux<float, float>(const Vecteur<float> &, entier);
template sptr<FiltreGen<cfloat>> filtre_rif_canaux<float, cfloat>(const Vecteur<float> &, entier);
template sptr<FiltreGen<cfloat>> filtre_rif_canaux<cfloat, cfloat>(const Vecteur<cfloat> &, entier);

template <typename Tc, typename T> sptr<FiltreGen<T>> filtre_rif_canaux(const Vecteur<Tc> &h, entier nb_canaux, MethodeRIF méthode)
{
  return std::make_shared<FiltreRIFCanauxGpu<T, Tc>>(h, nb_canaux, (int) méthode);
}
template sptr<FiltreGen<float>> filtre_rif_canaux<float, float>(const Vecteur<float> &, entier, MethodeRIF);
template sptr<FiltreGen<cfloat>> filtre_rif_canaux<float, cfloat>(const Vecteur<float> &, entier, MethodeRIF);
template sptr<FiltreGen<cfloat>> filtre_rif_canaux<cfloat, cfloat>(const Vecteur<cfloat> &, entier, MethodeRIF);

template <typename T> sptr<FiltreGen<T>> filtre_sois_canaux(const FRat<cfloat> &h, entier nb_canaux, tsd::filtrage::RIIStructure s)
{
  return std::make_shared<ChaineSOISCanauxGpu<T>>(h, nb_canaux, s);
}
template sptr<FiltreGen<float>> filtre_sois_canaux<float>(const FRat<cfloat> &, entier, tsd::filtrage::RIIStructure);
template sptr<FiltreGen<cfloat>> filtre_sois_canaux<cfloat>(const FRat<cfloat> &, entier, tsd::filtrage::RIIStructure);

}  // namespace tsd_amd
