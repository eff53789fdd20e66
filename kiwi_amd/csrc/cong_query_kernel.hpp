// Launch-side declarations of the CoNgram query kernels (cong_query_kernel.hip): the embedding-table queries of the reference's
// kiwi_cong_* API (src/CoNgramModel.cpp:2416-2745) for a batch of queries -- every candidate row scored with the shared formulas of
// flat_model.hpp (congCosine / congPredict / congPredictDiff), then the top N per query ordered by score descending, id ascending.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace kamd
{
	// query kinds (kamd_cong_topk's `kind`)
	enum CongQueryKind : uint32_t { CQ_SIMILAR_WORDS = 0, CQ_SIMILAR_CONTEXTS = 1, CQ_PREDICT = 2, CQ_PREDICT_DIFF = 3 };
	constexpr uint32_t kCongFusedTopN = 256;      // the largest N the selection kernel orders on the device

	struct CongQueryTables
	{
		const uint8_t* ctxEmb; const uint8_t* outEmb;     // the engine's device copies (rows: dim x s8, f32 scale, f32 bias / unused; stride dim + 8)
		const float* invNormOut; const float* invNormCtx; // congInvNorm of every row (similarity kinds)
		uint32_t dim, stride;
	};
	// nQ queries (ids / bg / weights: device arrays of nQ; bg and weights are read by CQ_PREDICT_DIFF only, every id valid) against candidates
	// [0, nCand): scores[q * nCand + i]
	void launchCongScores(const CongQueryTables& T, uint32_t kind, const uint32_t* ids, const uint32_t* bg, const float* weights, uint32_t nQ,
		uint32_t nCand, float* scores, hipStream_t stream);
	// the best topN (1 .. kCongFusedTopN, <= nCand) of every row of scores: outIds / outScores[q * topN + j]
	void launchCongTopN(const float* scores, uint32_t nQ, uint32_t nCand, uint32_t topN, uint32_t* outIds, float* outScores, hipStream_t stream);
}
