// cong_query_ref: the reference's CoNgram query functions (src/CoNgramModel.cpp:2416-2870, the model behind kiwi_cong_*) run on one cong.mdl, for the
// goldens of tests/test_cong_query_cpu.py and tests/test_gpu_cong_query.py (tools/make_golden_cong_query.py drives it).  The model is loaded the way the
// analysis pin loads it: CoNgramModelBase::create(mem, ArchType::sse4_1, useDistantTokens = (windowSize > 0), quantized = true).
//
//     usage:  cong_query_ref <cong.mdl>   < queries   > answers
//
// One query per input line, one answer line each:
//     W id n | C id n | P id n       mostSimilarWords / mostSimilarContexts / predictWordsFromContext -> count, then count pairs "id score"
//     D id bg weight n               predictWordsFromContextDiff                                         -> the same
//     S a b | T a b                  wordSimilarity / contextSimilarity                                  -> score
//     X k id...                      toContextId                                                          -> context id
//     M                              getContextWordMap                                                    -> one line per context: "ctx len ids..."
// Floats are printed as their bit patterns (%08x) so that the goldens hold them exactly.
// Build (tools/make_golden_cong_query.py): c++ -std=c++17 -O2 -I<kiwi>/include tools/cong_query_ref.cpp <libkiwi> -o cong_query_ref
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include <kiwi/Kiwi.h>      // (first: the headers CoNgramModel.h relies on)
#include <kiwi/CoNgramModel.h>

using namespace kiwi;

namespace
{
	struct Bytes
	{
		std::vector<char> v;
		const void* get() const { return v.data(); }
		size_t size() const { return v.size(); }
	};
	unsigned bits(float f) { unsigned u; std::memcpy(&u, &f, 4); return u; }
}

int main(int argc, char** argv)
{
	if (argc != 2) { std::fprintf(stderr, "usage: cong_query_ref <cong.mdl>\n"); return 2; }
	std::ifstream ifs{ argv[1], std::ios::binary };
	Bytes b{ std::vector<char>{ std::istreambuf_iterator<char>{ ifs }, std::istreambuf_iterator<char>{} } };
	if (b.v.size() < sizeof(lm::CoNgramModelHeader)) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
	lm::CoNgramModelHeader hd;
	std::memcpy(&hd, b.v.data(), sizeof(hd));
	auto model = lm::CoNgramModelBase::create(utils::MemoryObject{ std::move(b) }, ArchType::sse4_1, hd.windowSize > 0, true);
	std::string line;
	std::vector<std::pair<uint32_t, float>> out;
	while (std::getline(std::cin, line))
	{
		std::istringstream is{ line };
		char op = 0;
		is >> op;
		if (op == 'W' || op == 'C' || op == 'P' || op == 'D')
		{
			uint32_t id = 0, bg = 0; float w = 0; size_t n = 0;
			is >> id;
			if (op == 'D') is >> bg >> w;
			is >> n;
			out.assign(n + 1, {});
			size_t c = op == 'W' ? model->mostSimilarWords(id, n, out.data()) : op == 'C' ? model->mostSimilarContexts(id, n, out.data())
				: op == 'P' ? model->predictWordsFromContext(id, n, out.data()) : model->predictWordsFromContextDiff(id, bg, w, n, out.data());
			std::printf("%zu", c);
			for (size_t i = 0; i < c; ++i) std::printf(" %u %08x", out[i].first, bits(out[i].second));
			std::printf("\n");
		}
		else if (op == 'S' || op == 'T')
		{
			uint32_t a = 0, c = 0;
			is >> a >> c;
			std::printf("%08x\n", bits(op == 'S' ? model->wordSimilarity(a, c) : model->contextSimilarity(a, c)));
		}
		else if (op == 'X')
		{
			size_t k = 0; is >> k;
			std::vector<uint32_t> ids(k);
			for (auto& x : ids) is >> x;
			std::printf("%u\n", k ? model->toContextId(ids.data(), k) : 0u);
		}
		else if (op == 'M')
		{
			const auto map = model->getContextWordMap();
			std::printf("%zu\n", map.size());
			for (size_t c = 0; c < map.size(); ++c)
			{
				std::printf("%zu %zu", c, map[c].size());
				for (auto x : map[c]) std::printf(" %u", x);
				std::printf("\n");
			}
		}
		else { std::fprintf(stderr, "bad query: %s\n", line.c_str()); return 1; }
		std::fflush(stdout);
	}
	return 0;
}
