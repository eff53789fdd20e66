// CoNgram query kernels (kiwi_cong_* / kamd_cong_topk): the reference answers one query at a time on one CPU thread with a gemv over every
// vocabulary (or context) row and a partial_sort_copy of the whole score vector (src/CoNgramModel.cpp:2416-2745).  Here a batch of queries:
//   k_cong_scores : one lane per (query, candidate): the exact int32 dot of two s8 rows on v_dot4_i32_i8, then the fp32 epilogue of the kind
//                   (flat_model.hpp congCosine / congPredict / congPredictDiff, the same source the host paths use)
//   k_cong_topn   : one block per query: a radix select over the order keys (flat_model.hpp congOrderKey) finds the N-th best key, the
//                   candidates before it (and the lowest ids among those equal to it) are gathered in id order and sorted in LDS
// The order is total (score descending, then id ascending), so the result does not depend on the schedule.
#include "cong_query_kernel.hpp"
#include "flat_model.hpp"

namespace kamd
{
	namespace
	{
		constexpr uint32_t kBlock = 256, kWaves = kBlock / 64;
		constexpr uint32_t kMaxRowWords = 16 + 2;      // dim <= 64 (the loader's tables: 32 or 64) + scale + bias

		__device__ __forceinline__ int32_t dotRow(const uint32_t* q, const uint32_t* r, uint32_t nw)
		{
			int32_t acc = 0;
			for (uint32_t k = 0; k < nw; ++k) acc = __builtin_amdgcn_sdot4((int)q[k], (int)r[k], acc, false);      // v_dot4_i32_i8: exact
			return acc;
		}

		__global__ void __launch_bounds__(kBlock) k_cong_scores(CongQueryTables T, uint32_t kind, const uint32_t* ids, const uint32_t* bg, const float* weights,
			uint32_t nCand, float* scores)
		{
			__shared__ uint32_t qRow[kMaxRowWords], bRow[kMaxRowWords];
			const uint32_t q = blockIdx.y, nw = T.dim >> 2;
			const uint32_t id = ids[q];
			const uint8_t* qTable = kind == CQ_SIMILAR_WORDS ? T.outEmb : T.ctxEmb;
			const uint8_t* cTable = kind == CQ_SIMILAR_CONTEXTS ? T.ctxEmb : T.outEmb;
			if (threadIdx.x < nw + 2)
			{
				qRow[threadIdx.x] = reinterpret_cast<const uint32_t*>(qTable + (size_t)id * T.stride)[threadIdx.x];
				if (kind == CQ_PREDICT_DIFF) bRow[threadIdx.x] = reinterpret_cast<const uint32_t*>(T.ctxEmb + (size_t)bg[q] * T.stride)[threadIdx.x];
			}
			__syncthreads();
			const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
			if (i >= nCand) return;
			const uint32_t* r = reinterpret_cast<const uint32_t*>(cTable + (size_t)i * T.stride);      // rows start at 4-byte alignment (stride dim + 8)
			const int32_t dot = dotRow(qRow, r, nw);
			const float qScale = __uint_as_float(qRow[nw]), rScale = __uint_as_float(r[nw]);
			float s;
			if (kind == CQ_SIMILAR_WORDS || kind == CQ_SIMILAR_CONTEXTS)
			{
				const float* inv = kind == CQ_SIMILAR_WORDS ? T.invNormOut : T.invNormCtx;
				s = i == id ? -99999.f : congCosine(dot, qScale, rScale, inv[id], inv[i]);      // the query itself: "remove self"
			}
			else if (kind == CQ_PREDICT) s = congPredict(dot, qScale, rScale, __uint_as_float(qRow[nw + 1]));
			else
			{
				const int32_t dotBg = dotRow(bRow, r, nw);
				s = congPredictDiff(dot, dotBg, qScale, __uint_as_float(bRow[nw]), rScale, __uint_as_float(qRow[nw + 1]), __uint_as_float(bRow[nw + 1]), weights[q]);
			}
			scores[(size_t)q * nCand + i] = s;
		}

		// exclusive prefix count of `flag` over the block (lane order = thread order); total in *total.  Uses wcnt[kWaves].
		__device__ __forceinline__ uint32_t blockRank(bool flag, uint32_t* wcnt, uint32_t* total)
		{
			const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
			const uint64_t b = __ballot(flag);
			const uint32_t inWave = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
			if (lane == 0) wcnt[wave] = (uint32_t)__popcll(b);
			__syncthreads();
			uint32_t before = 0, all = 0;
			for (uint32_t w = 0; w < kWaves; ++w) { before += w < wave ? wcnt[w] : 0u; all += wcnt[w]; }
			__syncthreads();      // (wcnt is reused by the next call)
			*total = all;
			return before + inWave;
		}

		__global__ void __launch_bounds__(kBlock) k_cong_topn(const float* scores, uint32_t nCand, uint32_t topN, uint32_t* outIds, float* outScores)
		{
			__shared__ uint32_t hist[256];
			__shared__ uint32_t sPrefix, sNeed, wcnt[kWaves];
			__shared__ uint64_t sel[kBlock];
			const uint32_t q = blockIdx.x, t = threadIdx.x;
			const float* row = scores + (size_t)q * nCand;
			if (t == 0) { sPrefix = 0; sNeed = topN; }
			// radix select, 8 bits per pass from the top: the topN-th smallest key T; sNeed = how many of the keys equal to T belong to the result
			uint32_t mask = 0;
			for (int shift = 24; shift >= 0; shift -= 8)
			{
				hist[t] = 0;
				__syncthreads();
				const uint32_t prefix = sPrefix;
				for (uint32_t i = t; i < nCand; i += kBlock)
				{
					const uint32_t key = congOrderKey(row[i]);
					if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
				}
				__syncthreads();
				if (t == 0)
				{
					uint32_t need = sNeed, d = 0;
					for (; d < 255; ++d) { if (hist[d] >= need) break; need -= hist[d]; }
					sNeed = need; sPrefix = prefix | (d << shift);
				}
				mask |= 255u << shift;
				__syncthreads();
			}
			const uint32_t T = sPrefix, need = sNeed;
			// gather in id order: every key < T, and the first `need` ids with key == T -- exactly topN entries
			uint32_t nSel = 0, tiesSeen = 0;
			for (uint32_t base = 0; base < nCand; base += kBlock)
			{
				const uint32_t i = base + t;
				const uint32_t key = i < nCand ? congOrderKey(row[i]) : 0xFFFFFFFFu;
				const bool eq = i < nCand && key == T;
				uint32_t nEq, nTake;
				const uint32_t eqRank = blockRank(eq, wcnt, &nEq);
				const bool take = (i < nCand && key < T) || (eq && tiesSeen + eqRank < need);
				const uint32_t r = blockRank(take, wcnt, &nTake);
				if (take && nSel + r < kBlock) sel[nSel + r] = (uint64_t)key << 32 | i;
				nSel += nTake; tiesSeen += nEq;
			}
			for (uint32_t j = nSel + t; j < kBlock; j += kBlock) sel[j] = ~0ull;
			__syncthreads();
			// bitonic sort of the 256 (key, id) pairs
			for (uint32_t k = 2; k <= kBlock; k <<= 1)
				for (uint32_t j = k >> 1; j > 0; j >>= 1)
				{
					const uint32_t p = t ^ j;
					if (p > t)
					{
						const uint64_t a = sel[t], b = sel[p];
						const bool up = (t & k) == 0;
						if ((a > b) == up) { sel[t] = b; sel[p] = a; }
					}
					__syncthreads();
				}
			if (t < topN)
			{
				const uint32_t id = (uint32_t)sel[t];      // (always < nCand: exactly topN <= nCand entries were gathered)
				outIds[(size_t)q * topN + t] = id;
				outScores[(size_t)q * topN + t] = id < nCand ? row[id] : 0.f;
			}
		}
	}

	void launchCongScores(const CongQueryTables& T, uint32_t kind, const uint32_t* ids, const uint32_t* bg, const float* weights, uint32_t nQ,
		uint32_t nCand, float* scores, hipStream_t stream)
	{
		if (!nQ || !nCand) return;
		hipLaunchKernelGGL(k_cong_scores, dim3((nCand + kBlock - 1) / kBlock, nQ), dim3(kBlock), 0, stream, T, kind, ids, bg, weights, nCand, scores);
	}

	void launchCongTopN(const float* scores, uint32_t nQ, uint32_t nCand, uint32_t topN, uint32_t* outIds, float* outScores, hipStream_t stream)
	{
		if (!nQ || !topN) return;
		hipLaunchKernelGGL(k_cong_topn, dim3(nQ), dim3(kBlock), 0, stream, scores, nCand, topN, outIds, outScores);
	}
}
