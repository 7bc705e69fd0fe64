// Test driver of searchDisk's re-rank through the class surface (tests/test_gpu_rerank_class.py builds it with g++).
//   rerank_tool d nc code_size nsubc centroids info edges pq norm_pq opq|- index queries.fvecs nq k nprobe max_codes ef
//               pruning base.bvecs host|device|env out.bin
// Loads a Grouping index the way the reference's disk driver does (tests/test_ivfhnsw_grouping_sift1b_disk.cpp), then
// writes labels [searchDisk nq*k | searchDisk_batch(kc = 0) nq*k] followed by the distances in the same layout.
//   host    nothing loaded: the host loop reads the base file
//   device  upload_base(base) first
//   env     nothing loaded by the driver: IVFHNSW_RERANK=device (set by the caller) loads it at the first searchDisk
#include <ivf-hnsw/IndexIVF_HNSW_Grouping.h>

#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

using namespace ivfhnsw;

int main(int argc, char **argv)
try {
    if (argc != 22)
        throw std::runtime_error("usage: see the head of rerank_tool.cpp");
    const size_t d = atol(argv[1]), nc = atol(argv[2]), cs = atol(argv[3]), nsubc = atol(argv[4]);
    const char *centroids = argv[5], *info = argv[6], *edges = argv[7], *ppq = argv[8], *pnorm = argv[9], *popq = argv[10],
               *pindex = argv[11], *pqueries = argv[12];
    const size_t nq = atol(argv[13]), k = atol(argv[14]), nprobe = atol(argv[15]), max_codes = atol(argv[16]),
                 ef = atol(argv[17]);
    const bool pruning = atoi(argv[18]) != 0;
    const char *pbase = argv[19];
    const std::string mode = argv[20];
    IndexIVF_HNSW_Grouping *index = new IndexIVF_HNSW_Grouping(d, nc, cs, 8, nsubc);
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
    index->do_pruning = pruning;
    std::vector<float> q(nq * d);
    {
        std::ifstream in(pqueries, std::ios::binary);
        readXvec<float>(in, q.data(), d, nq);
    }
    if (mode == "device")
        index->upload_base(pbase);
    else if (mode != "host" && mode != "env")
        throw std::runtime_error("mode must be host, device or env");
    std::vector<long> lab(2 * nq * k);
    std::vector<float> dist(2 * nq * k);
    for (size_t i = 0; i < nq; i++)
        index->searchDisk(k, q.data() + i * d, dist.data() + i * k, lab.data() + i * k, pbase);
    index->searchDisk_batch(nq, k, q.data(), dist.data() + nq * k, lab.data() + nq * k, pbase);
    FILE *f = fopen(argv[21], "wb");
    if (!f)
        throw std::runtime_error("cannot write the result file");
    fwrite(lab.data(), sizeof(long), lab.size(), f);
    fwrite(dist.data(), sizeof(float), dist.size(), f);
    fclose(f);
    index->release_base();
    delete index;
    return 0;
} catch (const std::exception &e) {
    fprintf(stderr, "rerank_tool: %s\n", e.what());
    return 1;
}
