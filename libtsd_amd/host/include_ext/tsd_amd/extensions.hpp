// tsd_amd/extensions.hpp -- what the MI355X adaptors offer BEYOND libtsd's own API.  Nothing in
// libtsd's headers is changed to make room for these: they are free functions in namespace
// tsd_amd, declared against whichever "tsd/*.hpp" is on the include path (libtsd's or the mirror).
#pragma once
#include "tsd/tsd.hpp"
#include "tsd/filtrage.hpp"
#include "tsd/fourier.hpp"
#include <tuple>

namespace tsd_amd {
using namespace tsd;   // sptr / entier / cfloat: members of tsd in the mirror, global aliases in libtsd (fr.hpp, commun.hpp)

// ---- FFT plan hook (core/include/tsd/fourier.hpp:35, core/src/fourier/fourier.cc:469-481) ----------
// A FFTPlan on tsdgpu_fft.  installe_fftplan_gpu() assigns the factory to tsd::fourier::fftplan_defaut,
// after which every fft() / ifft() / tfrplan_création() / TFRCorrelateurBloc / Spectrum of libtsd
// runs its transforms on the GPU.  (The mirror's fftplan_defaut starts out as this factory.)
sptr<tsd::fourier::FFTPlan> fftplan_gpu();
void installe_fftplan_gpu();
// RTFRPlan on tsdgpu_rfft (packed half-size transform, untangling and forced symmetry fused on the device)
sptr<FiltreGen<float, cfloat>> rtfrplan_gpu(entier n = -1);

// ---- filtre_fft with a DEVICE-side spectral response ---------------------------------------------
// libtsd's OLA engine calls config.traitement_freq(X) on the host for every block.  When the
// processing is a product by a fixed response H (N values, N = the FFT size filtre_fft returns) this
// form keeps everything on the GPU: X *= H.  config.traitement_freq, when also set, still runs (after
// the product) through the host bridge.
std::tuple<sptr<Filtre<cfloat, cfloat, tsd::fourier::FiltreFFTConfig>>, entier>
filtre_fft_reponse(const tsd::fourier::FiltreFFTConfig &config, const Veccf &H);
// FFT size N the OLA engine picks for a configuration (what H must be sized to)
entier filtre_fft_dim(const tsd::fourier::FiltreFFTConfig &config);

// ---- several GPUs behind one operator object -----------------------------------------------------------
// filtre_rif / filtre_sois / filtre_itrp (hence filtrer, rééchan ...) cut a large host vector (>= 2^22
// samples) into one contiguous chunk per GPU of the node, each with its small halo, and run all devices
// at once (include/tsdgpu.h: tsdgpu_sharded_step_host).  Automatic when the process sees several GPUs;
// fixe_fragments(n) forces n logical shards (spread round-robin over the devices present; 0 or 1: off,
// -1: automatic again), like the environment variable TSD_AMD_SHARDS.
void fixe_fragments(int n);

// ---- channel banks: C streams of ONE filter in one object (include/tsdgpu.h: tsdgpu_fir_bank / tsdgpu_sos_bank) --------
// libtsd has no multichannel filter: these are extensions, not stand-ins.  step(x, y): x.rows() == nb_canaux * n, channel after
// channel (the storage of an n x nb_canaux Tab: Tab::map of a libtsd matrix works), y the same layout; host or resident
// vectors, in place allowed.  Each channel behaves as its own filtre_rif<Tc,T>(h) / filtre_sois<T>(h, s) object fed the same
// blocks (the FIR channels bit-identical to a direct-method filtre_rif; up to 12289 taps).
template <typename Tc, typename T> sptr<FiltreGen<T>> filtre_rif_canaux(const Vecteur<Tc> &h, entier nb_canaux);
// The same bank on a chosen scheme: RIF_DIRECTE is the two-argument form; RIF_OLS filters by overlap-save on 1024-point blocks
// (2 .. 961 taps; outside that range the direct scheme serves the request), each channel within 1e-5 of the reference's peak,
// aligned as the direct bank, a non-finite sample reaching its own blocks of its own channel only; RIF_AUTO chooses per step
// from the tap count and the block length (tsdgpu.h: tsdgpu_fir_bank_create_method).
enum MethodeRIF { RIF_AUTO = 0, RIF_DIRECTE = 1, RIF_OLS = 2 };      // (the values of tsdgpu_fir_method)
template <typename Tc, typename T> sptr<FiltreGen<T>> filtre_rif_canaux(const Vecteur<Tc> &h, entier nb_canaux, MethodeRIF méthode);
template <typename T>
sptr<FiltreGen<T>> filtre_sois_canaux(const FRat<cfloat> &h, entier nb_canaux,
                                      tsd::filtrage::RIIStructure s = tsd::filtrage::FormeDirecte2);

// ---- rate-changing channel banks: C streams through ONE integer-rate stage (include/tsdgpu.h: tsdgpu_polyfir_bank) ------
// The same extension for filtre_rif_decim / filtre_rif_demi_bande / filtre_rif_ups / decimateur.  step(x, y): x.rows() ==
// nb_canaux * n, channel after channel; y is resized to nb_canaux * n_out, same layout (all channels share one phase counter,
// hence one n_out); host or resident vectors.  Each channel behaves as its own single-stream object fed the same blocks.
// Served: the taps of all branches within 4096 floats and 257 R + K <= 16000 for a decimator (tsdgpu.h); else the factory fails.
template <typename Tc, typename T> sptr<FiltreGen<T>> filtre_rif_decim_canaux(const Vecteur<Tc> &h, entier R, entier nb_canaux);
template <typename Tc, typename T> sptr<FiltreGen<T>> filtre_rif_demi_bande_canaux(const Vecteur<Tc> &h, entier nb_canaux);
template <typename Tc, typename T> sptr<FiltreGen<T>> filtre_rif_ups_canaux(const Vecteur<Tc> &h, entier R, entier nb_canaux);
template <typename T> sptr<FiltreGen<T>> decimateur_canaux(entier R, entier nb_canaux);

// ---- polyphase channelizer: ONE wideband complex stream into nb_canaux channel rows (include/tsdgpu.h: tsdgpu_channelizer) ----
// The maximally decimated analysis bank: channel c (centre c / nb_canaux of the input rate) shifted to DC, filtered with the real
// prototype h, every nb_canaux-th sample kept; no normalisation.  step(x, y): x.rows() a whole number of nb_canaux-sample frames
// (else échec); y is resized to nb_canaux * (n / nb_canaux), channel after channel: what filtre_rif_canaux::step and the banks
// above take.  Host or resident vectors; x and y must be different vectors.  The channels of a frame share one transform: the
// error bound is 1e-5 of the peak over ALL channels, and a NaN / Inf in input frame f reaches every channel of output frames
// f .. f + ceil(K / nb_canaux) - 1.  Served: nb_canaux a power of two in [8, 1024], K <= 16 nb_canaux; else the factory fails.
sptr<FiltreGen<cfloat>> canaliseur_polyphase(const Vecf &h, entier nb_canaux);
// The same bank oversampled by surech = OS in {1, 2, 4}: a frame every D = nb_canaux / OS samples, so that each row keeps a clean
// band around its centre for a per-channel bank to filter and decimate.  step(x, y): x.rows() a whole number of hops of D samples
// (else échec); y is resized to nb_canaux * (n / D), channel after channel.  The object carries the history and the phase of the
// hop; a NaN / Inf at stream position q reaches every channel of output frames floor(q / D) .. floor((q + P nb_canaux) / D) - 1,
// P = ceil(K / nb_canaux).  Served: nb_canaux as above, K <= 16 D; else the factory fails.  surech = 1 is the factory above.
sptr<FiltreGen<cfloat>> canaliseur_polyphase(const Vecf &h, entier nb_canaux, entier surech);
// The maximally decimated bank for a REAL stream (tsdgpu_channelizer_create_real): rows 0 .. nb_canaux / 2 of canaliseur_polyphase on
// the widened stream; rows nb_canaux / 2 + 1 .. nb_canaux - 1 are the conjugates of rows nb_canaux / 2 - 1 .. 1 and are not
// produced.  step(x, y): x.rows() floats, a whole number of nb_canaux-sample frames (else échec); y is resized to
// (nb_canaux / 2 + 1) * (n / nb_canaux), channel after channel.  Host or resident vectors.  Rows 0 and nb_canaux / 2 come out with
// an imaginary part of exactly 0.  Served: nb_canaux a power of two in [16, 1024], K <= 16 nb_canaux; else the factory fails.
sptr<FiltreGen<float, cfloat>> canaliseur_polyphase_reel(const Vecf &h, entier nb_canaux);
// The same bank oversampled by surech = OS in {1, 2, 4} (tsdgpu_channelizer_create_real_oversampled): a frame every
// D = nb_canaux / OS floats, rows 0 .. nb_canaux / 2 of canaliseur_polyphase(h, nb_canaux, surech) on the widened stream.
// step(x, y): x.rows() floats, a whole number of hops of D (else échec); y is resized to (nb_canaux / 2 + 1) * (n / D), channel
// after channel.  The object carries the history and the phase of the hop.  Served: nb_canaux as above, K <= 16 D; else the
// factory fails (surech < 1 included).  surech = 1 is the factory above and its bits.
sptr<FiltreGen<float, cfloat>> canaliseur_polyphase_reel(const Vecf &h, entier nb_canaux, entier surech);

// ---- polyphase synthesizer: nb_canaux channel rows into ONE wideband complex stream (include/tsdgpu.h: tsdgpu_synthesizer) ----
// The maximally decimated synthesis bank, the dual of canaliseur_polyphase: channel c upsampled by nb_canaux, filtered at baseband
// with the real prototype h, shifted to c / nb_canaux of the output rate, the channels summed; no normalisation.  step(x, y):
// x.rows() = nb_canaux blocks of F samples, channel after channel (else échec): what canaliseur_polyphase::step and the banks
// above produce; y is resized to nb_canaux * F.  Host or resident vectors; x and y must be different vectors.  The samples of a
// frame share one transform: the error bound is 1e-5 of the peak of the step, and a NaN / Inf in input frame m reaches every
// sample of output frames m .. m + ceil(K / nb_canaux) - 1.  Served: nb_canaux a power of two in [8, 1024], K <= 16 nb_canaux.
sptr<FiltreGen<cfloat>> synthetiseur_polyphase(const Vecf &h, entier nb_canaux);
// The same bank oversampled by surech = OS in {1, 2, 4}, the way back from canaliseur_polyphase(h, nb_canaux, surech): a frame per
// hop of D = nb_canaux / OS output samples.  step(x, y): x.rows() = nb_canaux blocks of F samples (else échec); y is resized to
// D * F.  The object carries the history (the last ceil(K / D) - 1 frames) and the phase of the hop; a NaN / Inf in input frame m
// reaches every sample of output hops m .. m + ceil(K / D) - 1.  Served: nb_canaux as above, K <= 16 D; else the factory fails.
// surech = 1 is the factory above.
sptr<FiltreGen<cfloat>> synthetiseur_polyphase(const Vecf &h, entier nb_canaux, entier surech);
// The maximally decimated bank with a REAL output (tsdgpu_synthesizer_create_real), the way back from canaliseur_polyphase_reel:
// synthetiseur_polyphase on the block extended by the rows nb_canaux - c = conj(row c), whose output is real.  step(x, y):
// x.rows() = (nb_canaux / 2 + 1) blocks of F samples, channel after channel (else échec); y is resized to nb_canaux * F floats.
// Host or resident vectors.  The imaginary parts of rows 0 and nb_canaux / 2 are not used: any value there, a NaN included, leaves
// the output as it is.  Served: nb_canaux a power of two in [16, 1024], K <= 16 nb_canaux; else the factory fails.
sptr<FiltreGen<cfloat, float>> synthetiseur_polyphase_reel(const Vecf &h, entier nb_canaux);
// The same bank oversampled by surech = OS in {1, 2, 4} (tsdgpu_synthesizer_create_real_oversampled), the way back from
// canaliseur_polyphase_reel(h, nb_canaux, surech): a frame per hop of D = nb_canaux / OS floats, synthetiseur_polyphase(h, nb_canaux,
// surech) on the extended block.  step(x, y): x.rows() = (nb_canaux / 2 + 1) blocks of F samples (else échec); y is resized to
// D * F floats; x and y must not share memory.  The object carries the history (the last ceil(K / D) - 1 frames) and the phase of
// the hop.  Served: nb_canaux as above, K <= 16 D; else the factory fails (surech < 1 included).  surech = 1 is the factory above
// and its bits.
sptr<FiltreGen<cfloat, float>> synthetiseur_polyphase_reel(const Vecf &h, entier nb_canaux, entier surech);

// ---- device memory for resident vectors ------------------------------------------------------------
// A vector mapped on device memory, TabT<T,1>::map(ptr, n) (tableau.hpp:1067-1077), is accepted by
// every adaptor as input, and as output when it already has the size the step produces (resize() to
// the same size is a no-op in libtsd, tableau.cc:702-705): a chain filtre -> fft -> rééchan then
// never leaves the GPU.  These two wrap hipMalloc / hipFree so that C++ callers need no HIP headers.
void *alloue_gpu(size_t octets);
void libere_gpu(void *p);
void copie_vers_gpu(void *dst_gpu, const void *src_hote, size_t octets);
void copie_vers_hote(void *dst_hote, const void *src_gpu, size_t octets);
void synchronise_gpu();

}  // namespace tsd_amd
