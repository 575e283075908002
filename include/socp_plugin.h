/*
 * socp_plugin.h -- out-of-tree device models.
 *
 * The reference's plugin surface is a host C++ virtual (odeTools.hpp:82 Model, model.hpp:375 Control,
 * model.hpp:384 Hamiltonian); a virtual on the host cannot run inside a GPU kernel, so a model needs a
 * device twin.  In-tree models (goddard, doubleIntegrator, covid19) ship theirs; any other model class
 * provides one as a small plugin: a struct with the static device interface described in
 * socp_amd/csrc/plugin_impl.hpp, compiled by hipcc against this library's headers into a shared object.
 * The C++ mirror class of that model returns the plugin's id from model::DeviceModelId().
 *
 * Optional traits of the struct (plugin_impl.hpp lists them all).  Launch-table ABI 9 adds one:
 *   static constexpr int kEventChannels = K;                        (1 <= K <= 16)
 *   __device__ static double event_fn(const socp::ModelParams &P, double sw0, double sw1, double t, const double (&X)[S], int chan);
 * the scalars socp_events_batch (socp_hip.h) may watch along the trajectories, typically the switching function of the control
 * law; plain IEEE operations if a CPU restatement is to match bit for bit.  A model without it has no events entry in its table:
 * socp_ctx_event_channels says 0 and socp_events_batch returns SOCP_ERR_UNSUPPORTED (the in-tree example tests/plugin/lqr1d is
 * such a model).  A plugin built against an older launch table (ABI <= 8) is refused at registration: rebuild it.
 *
 * Launch-table ABI 10 adds the batched Jacobi-field launcher (socp_jacobi_batch, socp_hip.h).  It needs no trait: every model without
 * its own ComputeTraj gets it with no change to its source (kNoJacobi = true in the struct leaves the entry empty).  A plugin built
 * against an older launch table (ABI <= 9) is refused at registration: rebuild it.
 *
 * Launch-table ABI 11 adds the batched exact-fields launcher (socp_fields_batch, socp_hip.h) and its optional trait
 *   template <class T> __device__ static void rhs_t(const socp::ModelParams &P, double sw0, double sw1, double t, const T (&X)[S], T (&dX)[S]);
 * the right-hand side over a number type (socp_amd/csrc/dual.hpp), on plain IEEE operations; with T = double the bits of rhs.  A
 * model without it has no fields entry: socp_ctx_has_fields says 0 and socp_fields_batch returns SOCP_ERR_UNSUPPORTED
 * (tests/plugin/osc1d_fields_plugin.hip has the trait, the other example plugins do not).  A plugin built against an older launch
 * table (ABI <= 10) is refused at registration: rebuild it.
 *
 * Launch-table ABI 12 adds the batched extrema launcher (socp_extrema_batch, socp_hip.h).  It needs no trait: every model gets it
 * beside its trace entry with no change to its source, and a model with the event-channel trait has its channels among the
 * reduced ones.  A plugin built against an older launch table (ABI <= 11) is refused at registration: rebuild it.
 *
 * Launch-table ABI 13 adds the batched exact shooting-Jacobian launcher (socp_exact_jacobian_batch, socp_hip.h) and, beside rhs_t, its
 * optional traits
 *   template <class T> __device__ static T hamiltonian_t(const socp::ModelParams &P, double sw0, double sw1, double t, const T (&X)[S]);
 *   template <class T> __device__ static T switching_fn_t(const socp::ModelParams &P, double sw0, double sw1, double t, const T (&X)[S],
 *                                                         const T (&Xp)[S]);
 *   static constexpr bool kSwitchingReadsXp = ...;   // true: the row is H(t, X) - H(t, Xp) (model.hpp's default); false / absent: Xp is not read
 * with T = double the bits of hamiltonian / switching_fn.  A model gets the entry when it has all three traits, no switching_state hook,
 * no custom final rows and no ComputeTraj of its own (tests/plugin/osc1d_exact_jacobian_plugin.hip); otherwise
 * socp_ctx_has_exact_jacobian says 0 and the call returns SOCP_ERR_UNSUPPORTED.  A plugin built against an older launch table
 * (ABI <= 12) is refused at registration: rebuild it.
 *
 * Launch-table ABI 14 adds the batched observables launcher (socp_observe_batch, socp_hip.h) and its optional trait
 *   static constexpr int kObservables = NO;                         (1 <= NO <= 16)
 *   static constexpr const char *kObservableNames[NO] = {...};
 *   __device__ static void observe(const socp::ModelParams &P, double sw0, double sw1, double t, const double (&X)[S],
 *                                  const double (&u)[NU], double (&y)[NO]);
 * scalars of one row of a trajectory -- a drag, a clearance, a norm -- whose extrema and trapezoid integrals the library reduces
 * over the rows of every segment.  u is control_only at the row, evaluated once by the kernel with the row's aux pair; plain IEEE
 * operations if a CPU restatement is to match bit for bit.  A model without the trait, or with its own ComputeTraj, has no observe
 * entry: socp_ctx_has_observe says 0 and socp_observe_batch returns SOCP_ERR_UNSUPPORTED (tests/plugin/osc1d_observe_plugin.hip
 * has the trait, the other example plugins do not).  A plugin built against an older launch table (ABI <= 13) is refused at
 * registration: rebuild it.
 *
 * Launch-table ABI 15 adds the batched exact-sensitivities launcher (socp_sensitivity_batch, socp_hip.h).  Its trait is a way of
 * writing the three traits of ABI 13: generic in the PARAMETER view as well,
 *   template <class T, class PV> __device__ static void rhs_t(const PV &P, double sw0, double sw1, double t, const T (&X)[S], T (&dX)[S]);
 *   template <class T, class PV> __device__ static T hamiltonian_t(const PV &P, double sw0, double sw1, double t, const T (&X)[S]);
 *   template <class T, class PV> __device__ static T switching_fn_t(const PV &P, double sw0, double sw1, double t, const T (&X)[S],
 *                                                                   const T (&Xp)[S]);
 * where PV is anything with p[i]: socp::ModelParams (the texts are then what they were) or the dual view of a parameter block.  A
 * local that holds a parameter is `auto`, a comparison reads d_val (tests/plugin/osc1d_sensitivity_plugin.hip).  A model whose traits
 * take socp::ModelParams only keeps its fields and exact-Jacobian entries and has no sensitivity entry: socp_ctx_has_sensitivity says 0
 * and the call returns SOCP_ERR_UNSUPPORTED.  A plugin built against an older launch table (ABI <= 14) is refused at registration:
 * rebuild it.
 *
 * Launch-table ABI 16 adds the Hamiltonian-gradient launcher (socp_hamiltonian_gradient_batch, socp_hip.h).  Its trait is hamiltonian_t
 * alone, in either of the two ways above: any model that has it gets the entry.
 *   CHECKING A HAND-WRITTEN MODEL.  The call returns G = (dH/dp, -dH/dx) of the model's own Hamiltonian text, by dual numbers, at the
 * points socp_eval_batch takes; compare it with SOCP_EVAL_RHS at states on every arc of the control law.  The two agree to rounding
 * where the law minimises H over a set that does not depend on the state (socp_hip.h says what G is otherwise); a row that is off
 * by more than rounding is a derivation error in rhs or in hamiltonian -- or a property to write down, as covid19's rows 4 and 6 are.
 *   A MODEL FROM ITS HAMILTONIAN.  A struct that brings only D, S, NU, kRefOrder, control_only and hamiltonian_t (T = double must
 * work: it is the model's Hamiltonian) becomes a whole model through
 *   SOCP_DEFINE_HAMILTONIAN_PLUGIN(MODEL_ID, MDL, NPARAMS, STEP_NBR, {defaults})
 * which registers socp::plugin::FromHamiltonian<MDL> (socp_amd/csrc/hamiltonian_model.hpp): rhs = that gradient, hamiltonian =
 * hamiltonian_t<double>, switching_fn = H(t, X-) - H(t, X+) unless MDL has one; event channels, observables and a switching_fn of
 * MDL's own pass through.  Trajectories, residuals, FD Jacobians, hybrd sweeps, trace, cost, move, extrema, events and observe then
 * run through the unchanged launch-table kernels (tests/plugin/osc1d_h_plugin.hip, dint_h_plugin.hip).  Build with
 * -ffp-contract=off.  Such a model has no rhs_t -- the gradient of a gradient needs nested dual numbers -- so it has no fields,
 * exact-Jacobian or sensitivity entry and no variational equations; a right-hand side costs (1 + S) x the operations of H.  An
 * optional hint `static constexpr int kGradientWidth = W;` cuts the S directions into passes of W (registers against time, never a
 * bit).  A plugin built against an older launch table (ABI <= 15) is refused at registration: rebuild it.
 *
 * Launch-table ABI 17 adds the Hamiltonian-Jacobian launcher (socp_hamiltonian_jacobian_batch, socp_hip.h: A = dG/dX of that gradient,
 * by NESTED dual numbers).  Its trait is a hamiltonian_t that instantiates on socp::DualN<W, socp::Dual> as well, which every text
 * written as above does: + - * /, d_sqrt, d_abs, d_exp, d_val, plain doubles and parameters.  Any model that has it gets the entry.
 *   A MODEL FROM ITS HAMILTONIAN, WITH THE EXACT ENTRIES.  The same struct becomes a model with exact fields, the exact shooting
 * Jacobian (and socp_newton_batch with jac = 2 on it) through
 *   SOCP_DEFINE_HAMILTONIAN_PLUGIN_EXACT(MODEL_ID, MDL, NPARAMS, STEP_NBR, {defaults})
 * which registers socp::plugin::FromHamiltonianExact<MDL>: everything FromHamiltonian gives, plus rhs_t<T, PV> = the gradient taken on
 * the carrier T (T = double: rhs itself; T = Dual: nested numbers, whose value parts are rhs's bits), hamiltonian_t = MDL's own text,
 * and switching_fn_t = H(t, X-) - H(t, X+) with kSwitchingReadsXp = true unless MDL has a switching_fn of its own -- it then brings
 * its switching_fn_t (and kSwitchingReadsXp) too, or has no exact-Jacobian entry.  With hamiltonian_t generic in the parameter view
 * (template <class T, class PV>, ABI 15) the model has exact sensitivities too; with the one-argument form it has fields and the
 * exact Jacobian only (tests/plugin/osc1d_hx_plugin.hip, dint_hx_plugin.hip).  It is opt-in because it costs: a right-hand side over
 * dual numbers is (1 + S) evaluations of H on numbers of 2 (1 + W) doubles, and the exact kernels keep an RK4 step's states beside
 * them -- choose `static constexpr int kNestedGradientWidth = W;` for registers (the pass width of the gradient on dual numbers;
 * without it kGradientWidth, else S.  Every pass recomputes the value part, so the plain right-hand side is best left at one pass).  SOCP_DEFINE_HAMILTONIAN_PLUGIN keeps meaning what it meant.  A plugin built against
 * an older launch table (ABI <= 16) is refused at registration: rebuild it.
 *
 * Launch-table ABI 18 adds the neighbouring-extremal gain launcher (socp_gain_batch, socp_hip.h: the feedback gains dp/dx along every
 * row).  It needs no new trait: a model with rhs_t and none of switching_state, custom final rows or its own ComputeTraj gets the
 * entry with no source change, FromHamiltonianExact models included.  A plugin built against an older launch table (ABI <= 17) is
 * refused at registration: rebuild it.
 *
 * Launch-table ABI 19 adds the launcher of the same gains with a FREE final time (socp_gain_free_batch, socp_hip.h: dp/dx and dt_f/dx
 * by a bordered sweep).  It needs no new trait either: a model that has the gain entry and the hamiltonian_t trait gets it with no
 * source change.  A plugin built against an older launch table (ABI <= 18) is refused at registration: rebuild it.
 *
 * Launch-table ABI 20 adds the closed-loop guidance launcher, entry `guide` (socp_guide_batch, socp_hip.h: K dispersed cases per row
 * flown under the sampled neighbouring-extremal law).  It needs no trait at all beside rhs: every model without a switching_state hook,
 * custom final rows or its own ComputeTraj gets the entry with no source change, and the plugin's own build flags decide its
 * arithmetic.  The call asks for the gain entry of the problem's structure as well, so that its tables can exist.  A plugin built
 * against an older launch table (ABI <= 19) is refused at registration: rebuild it.
 *
 * Model ids below SOCP_PLUGIN_ID_MIN are reserved for in-tree models.
 */
#ifndef SOCP_PLUGIN_H_
#define SOCP_PLUGIN_H_

#ifdef __cplusplus
extern "C" {
#endif

#define SOCP_PLUGIN_ID_MIN 100

/* dlopen `path`, call its socp_plugin_register(); returns SOCP_OK or a negative SOCP_ERR_* */
int socp_plugin_load(const char *path);

/* called BY the plugin: `table` is a socp::ModelLaunchers (launch.hpp) of `table_bytes` bytes */
int socp_register_model(int model_id, const void *table, int table_bytes);

/* Every plugin exports `int socp_plugin_register(void)` -- generated by SOCP_DEFINE_MODEL_PLUGIN in
 * socp_amd/csrc/plugin_impl.hpp; it is the symbol socp_plugin_load looks up (not a symbol of this library). */

#ifdef __cplusplus
}
#endif
#endif
