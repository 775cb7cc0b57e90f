/* ttrl_qnet.h — the fused MultiLayerPerceptron / DuelingNetwork Q-value forward and acting.
 *
 * An addition to the C ABI of ttrl_mi355x.h (same library, same error codes, TTRL_ABI_VERSION
 * unchanged): the value networks of the reference's baseline.json ([128, 128] on the flattened
 * Kinematics observation), grid.json ([48, 48] on the flattened OccupancyGrid) and model_factory's
 * DuelingNetwork with its default empty heads (ttrl_agent/agents/common/models.py:50-104), as one
 * launch with the epsilon-greedy epilogue of ttrl_ego_attention_act.
 *
 * The network: float32; an observation row of `in` floats; n_layers hidden Linear + ReLU layers of
 * widths[l] units; then the head
 *   dueling 0   predict: q = h W + b                                  [last][A]
 *   dueling 1   value.predict and advantage.predict on the same h:    [last][A + 1]
 *               q = value + advantage - mean(advantage), in that order
 * Supported: 1 <= in <= 1024; 1 <= n_layers <= 3; every width a multiple of 16 in [16, 128];
 * 1 <= n_actions <= 16 (<= 15 with dueling).  Sizes that describe no network (a count or width
 * below 1, null pointers, dueling not 0 / 1) return TTRL_E_ARG, a network outside the domain
 * TTRL_E_UNSUPPORTED, both before anything is launched.
 *
 * Packed weights (floats, in order), every matrix as [in][out] (torch's Linear.weight transposed):
 *   layer l = 0 .. n_layers-1:  W_l [in_l][widths[l]], b_l [widths[l]]      (in_0 = in, in_l = widths[l-1])
 *   head, dueling 0:            predict W [last][A], b [A]
 *   head, dueling 1:            W [last][A + 1], b [A + 1]: columns 0 .. A-1 advantage.predict,
 *                               column A value.predict
 */
#ifndef TTRL_QNET_H
#define TTRL_QNET_H

#include "ttrl_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The packed length in floats, or the error code (negative) of an unsupported network. */
int64_t ttrl_mlp_sizes(int32_t in, int32_t n_layers, const int32_t* widths, int32_t n_actions, int32_t dueling);

/* q [batch][n_actions] for obs [batch][in] (device pointers; widths is a host array).  batch 0 is
 * TTRL_OK with no launch. */
int ttrl_mlp_q(const float* obs, int32_t batch, int32_t in, int32_t n_layers, const int32_t* widths,
               const float* weights, int32_t n_actions, int32_t dueling, float* q, void* stream);

/* The same forward with AbstractDQNAgent.act's epsilon-greedy choice in the same launch; every
 * argument after `dueling` as in ttrl_ego_attention_act: actions = np.argmax(q[e]) (first maximum,
 * first NaN), replaced with probability epsilon by a uniform action; Philox4x32-10 keyed on seed
 * with counter (env_offset + e, step), so for equal (seed, env, step, epsilon, n_actions) and an
 * equal greedy action both entry points pick the same action.  epsilon in [0, 1], env_offset >= 0,
 * actions / actions32 not both NULL. */
int ttrl_mlp_act(const float* obs, int32_t batch, int32_t in, int32_t n_layers, const int32_t* widths,
                 const float* weights, int32_t n_actions, int32_t dueling, float epsilon, const float* epsilon_dev,
                 uint64_t seed, int64_t step, const int64_t* step_dev, int64_t env_offset, float* q,
                 int64_t* actions, int32_t* actions32, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TTRL_QNET_H */
