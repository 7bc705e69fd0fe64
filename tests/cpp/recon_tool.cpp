// Test driver of IndexIVF_HNSW::reconstruct_labels / search_and_reconstruct through the class surface
// (tests/test_recon_classes.py builds it with g++).  KIND is ivf (IndexIVF_HNSW) or grouping (IndexIVF_HNSW_Grouping).
//   recon_tool KIND d nc code_size nsubc centroids info edges pq norm_pq opq|- in.index queries.fvecs nq k nprobe
//              max_codes ef pruning labels.u32 out.bin
//       out.bin: reconstruct_labels of labels.u32 [n][d] (float); search_and_reconstruct_batch of the nq queries:
//       distances [nq*k] (float), labels [nq*k] (int64), recons [nq*k][d] (float); search_and_reconstruct of query 0:
//       distances [k], labels [k], recons [k][d].
#include <ivf-hnsw/IndexIVF_HNSW_Grouping.h>

#include <cstdio>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

using namespace ivfhnsw;

static std::vector<IndexIVF_HNSW::idx_t> read_u32(const char *path)
{
    std::ifstream in(path, std::ios::binary);
    if (!in)
        throw std::runtime_error(std::string("cannot open ") + path);
    in.seekg(0, std::ios::end);
    const size_t n = (size_t)in.tellg() / sizeof(uint32_t);
    in.seekg(0);
    std::vector<IndexIVF_HNSW::idx_t> v(n);
    in.read(reinterpret_cast<char *>(v.data()), n * sizeof(uint32_t));
    return v;
}

int main(int argc, char **argv)
try {
    if (argc != 22)
        throw std::runtime_error("usage: see the head of recon_tool.cpp");
    const std::string kind = argv[1];
    const size_t d = atol(argv[2]), nc = atol(argv[3]), cs = atol(argv[4]), nsubc = atol(argv[5]);
    const char *centroids = argv[6], *info = argv[7], *edges = argv[8], *ppq = argv[9], *pnorm = argv[10], *popq = argv[11],
               *pindex = argv[12], *pqueries = argv[13];
    const size_t nq = atol(argv[14]), k = atol(argv[15]), nprobe = atol(argv[16]), max_codes = atol(argv[17]),
                 ef = atol(argv[18]);
    const bool pruning = atoi(argv[19]) != 0;
    IndexIVF_HNSW *index;
    if (kind == "grouping")
        index = new IndexIVF_HNSW_Grouping(d, nc, cs, 8, nsubc);
    else if (kind == "ivf")
        index = new IndexIVF_HNSW(d, nc, cs, 8);
    else
        throw std::runtime_error("KIND must be ivf or grouping");
    index->build_quantizer(centroids, info, edges, 16, 500);
    index->do_opq = strcmp(popq, "-") != 0;
    delete index->pq;
    index->pq = faiss::read_ProductQuantizer(ppq);
    if (index->do_opq)
        index->opq_matrix = dynamic_cast<faiss::LinearTransform *>(faiss::read_VectorTransform(popq));
    delete index->norm_pq;
    index->norm_pq = faiss::read_ProductQuantizer(pnorm);
    index->read(pindex);
    if (index->do_opq)
        index->rotate_quantizer();
    index->nprobe = nprobe;
    index->max_codes = max_codes;
    index->quantizer->efSearch = ef;
    if (auto *g = dynamic_cast<IndexIVF_HNSW_Grouping *>(index))
        g->do_pruning = pruning;
    std::vector<float> q(nq * d);
    {
        std::ifstream in(pqueries, std::ios::binary);
        readXvec<float>(in, q.data(), d, nq);
    }
    FILE *f = fopen(argv[21], "wb");
    if (!f)
        throw std::runtime_error("cannot write the result file");
    const std::vector<IndexIVF_HNSW::idx_t> lab = read_u32(argv[20]);
    std::vector<float> x(lab.size() * d);
    index->reconstruct_labels(lab.size(), lab.data(), x.data());
    fwrite(x.data(), sizeof(float), x.size(), f);
    std::vector<float> dist(nq * k), rec(nq * k * d);
    std::vector<long> labels(nq * k);
    index->search_and_reconstruct_batch(nq, k, q.data(), dist.data(), labels.data(), rec.data());
    fwrite(dist.data(), sizeof(float), dist.size(), f);
    fwrite(labels.data(), sizeof(long), labels.size(), f);
    fwrite(rec.data(), sizeof(float), rec.size(), f);
    index->search_and_reconstruct(k, q.data(), dist.data(), labels.data(), rec.data());
    fwrite(dist.data(), sizeof(float), k, f);
    fwrite(labels.data(), sizeof(long), k, f);
    fwrite(rec.data(), sizeof(float), k * d, f);
    fclose(f);
    delete index;
    return 0;
} catch (const std::exception &e) {
    fprintf(stderr, "recon_tool: %s\n", e.what());
    return 1;
}
